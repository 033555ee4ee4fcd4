"""The update tail on the GPU: what runs after the tile records (tests/update_tail_util.py; every case is proven on the CPU first by
tests/test_update_tail_oracle.py). Needs an MI355X: every test is marked `gpu`.

A. The record tree at fold depths 0 to 3: synthetic records through mppi_shard_finish against the fp64 formula (beta exact, eta within
ETA_RTOL, u and U' within U_TOL, the stored sequence the shift of U'), and the second fold level end to end at K = 2^20 + 1 with needles.
B. Action limits and the sequence filter on every path that applies the update, against clip / savgol_filter of the fp64 oracle's update.
"""
import numpy as np
import pytest

import needle_util as nu
import update_tail_util as ut

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


# =============================================================== A1: synthetic records at every depth of the tree
def test_shard_finish_refuses_records_its_scratch_cannot_fold(m):
    """a handle of 3 tiles has scratch for ceil(128/16) = 8 folded records: more than 1024 records whose fold needs more are refused with
    MPPI_ERR_INVALID_ARG before anything is launched (the records are never read: the sequence and the step counter stay as they were)"""
    import torch
    h, H, a = ut.tree_handle(m, 1)
    assert not ut.tree_fits(1025, 192) and not ut.tree_fits(20000, 192) and ut.tree_fits(1024, 192)
    U = ut.tree_U(H, a)
    h.set_action_sequence(U)
    recs, u = torch.zeros(8 * (2 + H * a), device="cuda"), torch.zeros(a, device="cuda")  # (a refused call reads none of it)
    torch.cuda.synchronize()
    for n in (1025, 20000):
        with pytest.raises(m.MppiError) as e:
            h.shard_finish(recs.data_ptr(), n, u.data_ptr())
        assert e.value.status == m._lib.ERR_INVALID_ARG and "mppi_shard_finish" in str(e.value) and str(n) in str(e.value), str(e.value)
        h.synchronize()
        np.testing.assert_array_equal(h.get_action_sequence(), U)
        assert h.get_step_counter() == 0 and not u.cpu().numpy().any()
    h.close()


@pytest.mark.parametrize("n", ut.TREE_N, ids=["n%d" % n for n in ut.TREE_N])
def test_record_tree_at_every_depth(m, n):
    """column_combine and k_combine_group alone: n synthetic records, the plain population and a needle record at every group edge"""
    h, H, a = ut.tree_handle(m, n)
    seen = {}
    for bstar in [None] + ut.tree_needles(n):
        ut.run_tree(m, h, H, a, n, bstar, seen)
    print("n = %d, %d fold levels | max eta error %.3g | max |dU'| %.3g" % (n, ut.tree_levels(n), seen["eta"], seen["dU"]))
    h.close()


# =============================================================== A2: the second fold level end to end
@pytest.mark.parametrize("case", ut.TWO_LEVEL, ids=nu.ids(ut.TWO_LEVEL))
def test_needle_reaches_the_update_through_two_fold_levels(m, case):
    """K = 2^20 + 1: 16385 tile records fold to 1025 and then to 65 (k_combine_group reading its own row-major output); needles in the tiles
    whose record slots are the group edges of both levels, and the lone sample of the last tile; with normalizeCost the step's temperature
    must reach both levels"""
    h, seen = nu.run_lone(m, case)
    assert ut.tree_levels(ut.K20_NB) == 2
    print("%s | min w_ref %.9f | min leave-one-out %.3g | max eta error %.3g" % (h.rollout_kernel_name(), seen["w"], seen["loo"], seen["eta"]))
    h.close()


# =============================================================== B: limits and filter on every path that applies the update
def report(case, seen):
    print("%s | max|dU'| %.3g (x scale)%s" % (case["id"], seen["dU"], " | filtered sequence at most %.3g of its bar" % seen["dS"] if "dS" in seen else ""))


@pytest.mark.parametrize("case", ut.OPTION_LONE, ids=nu.ids(ut.OPTION_LONE))
def test_limits_and_filter_on_a_lone_handle(m, case):
    """the column waves of the one-launch step, k_finish_cols at 3 and 129 tiles and behind a fold level, normalizeCost on two passes and on
    the tile kernel, the tile route with injected noise (R = 64 with the window the whole horizon, R = 32), a learned model, the Fossen AUV
    on both its kernels, a = 1"""
    report(case, ut.run_lone_options(m, case))


def test_a_filter_of_one_tap_leaves_the_sequence_alone(m):
    """window 1, order 0 is the identity: the stored sequence is the shift of U' bit for bit, on the route a filter takes (two launches)"""
    case = dict(ut.OPTION_CASES[-1], filter=(1, 0))
    h = ut.option_handle(m, case)
    for _ in range(ut.STEPS):
        h.next(case["x"])
        np.testing.assert_array_equal(h.get_action_sequence(), ut.shifted(h.debug_get(m.DBG_U_UPDATED)))
    assert np.abs(h.get_action_sequence()).max() > 100 * nu.U_TOL
    h.close()


@pytest.mark.parametrize("case", ut.OPTION_BY_PATH["shards3"], ids=nu.ids(ut.OPTION_BY_PATH["shards3"]))
def test_limits_and_filter_on_a_sharded_finish(m, case):
    """three shards in one process: partial -> gather by hand -> mppi_shard_finish; every shard's u, U' and stored sequence are the
    others' bits, and within the bars of the reference over all K samples"""
    import torch
    n, a = 3, case["a"]
    hs = [ut.option_handle(m, case, shard_rank=g, shard_count=n) for g in range(n)]
    assert sum(h.k_local for h in hs) == case["K"]
    _, p64 = ut.option_problems(case)
    rs, seen = hs[0].record_size, {}
    xd, recs, us = torch.tensor(case["x"], device="cuda"), torch.zeros(n * rs, device="cuda"), [torch.zeros(a, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    for s in range(ut.STEPS):
        U = hs[0].get_action_sequence()
        for g, h in enumerate(hs):
            h.shard_partial(xd.data_ptr(), recs[g * rs:(g + 1) * rs].data_ptr())
            h.synchronize()
        for g, h in enumerate(hs):
            h.shard_finish(recs.data_ptr(), n, us[g].data_ptr())
            h.synchronize()
        for g in range(1, n):
            np.testing.assert_array_equal(us[g].cpu().numpy(), us[0].cpu().numpy())
            ut.assert_same_state(m, hs[g], hs[0], "shard %d step %d" % (g, s), costs=False)
        eps = np.concatenate([h.debug_get(m.DBG_NOISE) for h in hs])
        ut.check_step(m, case, hs[0], p64, U, eps, us[0].cpu().numpy(), s, seen)
    report(case, seen)
    for h in hs:
        h.close()


@pytest.mark.parametrize("case", ut.OPTION_BY_PATH["p2p2"], ids=nu.ids(ut.OPTION_BY_PATH["p2p2"]))
def test_limits_on_the_direct_exchange(m, case):
    """two shards in one process exchange their records inside k_finish_cols_xchg: the bits of the all-gather path with the same limits,
    and within the bars of the reference"""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    n, a = 2, case["a"]
    ref = [ut.option_handle(m, case, shard_rank=g, shard_count=n) for g in range(n)]
    hs = [ut.option_handle(m, case, shard_rank=g, shard_count=n) for g in range(n)]
    ptrs = [h.p2p_export(want_ipc=False)[0] for h in hs]
    for h in hs:
        h.p2p_attach(ptrs, timeout_ms=500)
    with ThreadPoolExecutor(n) as ex:  # a probe synchronises its stream: all ranks must be in flight together
        assert all(ex.map(lambda h: h.p2p_probe(), hs))
    _, p64 = ut.option_problems(case)
    rs, seen = ref[0].record_size, {}
    xd, recs, u_ref = torch.tensor(case["x"], device="cuda"), torch.zeros(n * rs, device="cuda"), torch.zeros(a, device="cuda")
    us = [torch.zeros(a, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    for s in range(ut.STEPS):
        U = ref[0].get_action_sequence()
        for g, h in enumerate(ref):
            h.shard_partial(xd.data_ptr(), recs[g * rs:(g + 1) * rs].data_ptr())
            h.synchronize()
        for h in ref:
            h.shard_finish(recs.data_ptr(), n, u_ref.data_ptr())
            h.synchronize()
        for g, h in enumerate(hs):  # enqueue only: the kernels of both shards meet on the GPU
            h.p2p_step(xd.data_ptr(), us[g].data_ptr())
        for h in hs:
            h.synchronize()
            assert not h.p2p_timed_out()
        for g, h in enumerate(hs):
            np.testing.assert_array_equal(us[g].cpu().numpy(), u_ref.cpu().numpy())
            ut.assert_same_state(m, h, ref[g], "shard %d step %d" % (g, s))
        eps = np.concatenate([h.debug_get(m.DBG_NOISE) for h in hs])
        ut.check_step(m, case, hs[0], p64, U, eps, us[0].cpu().numpy(), s, seen)
    report(case, seen)
    for h in ref + hs:
        h.close()


@pytest.mark.parametrize("case", ut.OPTION_BY_PATH["pre"], ids=nu.ids(ut.OPTION_BY_PATH["pre"]))
def test_limits_on_the_prelaunched_step(m, case):
    """the one place where the clipped U' travels to the next step as granules (ugr_out of the column waves up to 128 tiles, FinishPre of
    k_finish_cols above): after 1, 2, 3 and 9 device steps u, the sequence, the costs and the step counter are a plain handle's bits, and
    the last step of each run is within the bars of the reference"""
    a = case["a"]
    hp, h0 = ut.option_handle(m, case), ut.option_handle(m, dict(case, tuning=None, kernel=("", "")))
    _, p64 = ut.option_problems(case)
    total, seen = 0, {}
    for n in case["counts"]:
        ut.device_steps(h0, case["x"], n - 1, a)
        U = h0.get_action_sequence()  # what the last step of this run starts from
        u0, up = ut.device_steps(h0, case["x"], 1, a), ut.device_steps(hp, case["x"], n, a)
        total += n
        np.testing.assert_array_equal(up, u0, err_msg="after %d steps" % total)
        ut.assert_same_state(m, hp, h0, "after %d steps" % total)
        assert hp.get_step_counter() == total
        ut.check_step(m, case, hp, p64, U, hp.debug_get(m.DBG_NOISE), up, total - 1, seen)
    report(case, seen)
    hp.close(); h0.close()


# =============================================================== mode changes: a filter takes the one-launch and the pre-launched step away
MODE = dict(ut.OPTION_CASES[0], kernel=("", ""), tuning=None, limits=False, filter=None)
STEP_PC, ROLLOUT_PC = "mppi::k_step_pc<2, ", "mppi::k_rollout_pc<2, "


def both(hs, call):
    for h in hs:
        call(h)


def test_filter_and_limits_switched_on_and_off_on_a_one_launch_handle(m):
    """(i) a one-launch handle and a plain two-launch handle receive the same calls: steps, a filter on, limits on, limits off, the filter
    off; the one-launch handle steps aside for the filter (k_rollout_pc) and comes back (k_step_pc); the same bits throughout"""
    h1, h2 = ut.option_handle(m, MODE), ut.option_handle(m, dict(MODE, tuning={"fused_step": 0}))
    hs, x, lim, n = (h1, h2), MODE["x"], ut.LIM_192, 0

    def steps(name1):
        nonlocal n
        assert h1.rollout_kernel_name().startswith(name1) and h2.rollout_kernel_name().startswith(ROLLOUT_PC), (h1.rollout_kernel_name(), h2.rollout_kernel_name())
        for _ in range(2):
            n += 1
            np.testing.assert_array_equal(h1.next(x), h2.next(x), err_msg="step %d" % n)
            ut.assert_same_state(m, h1, h2, "step %d" % n)
    steps(STEP_PC)
    both(hs, lambda h: h.set_sequence_filter(5, 3))
    steps(ROLLOUT_PC)
    both(hs, lambda h: h.set_action_limits(lim["lo"], lim["hi"]))
    steps(ROLLOUT_PC)
    both(hs, lambda h: h.set_sequence_filter(0))
    steps(STEP_PC)
    U = h1.get_action_sequence()[:-1]  # (the last row is the zero row the shift appends)
    assert (U >= np.asarray(lim["lo"], F32)).all() and (U <= np.asarray(lim["hi"], F32)).all()
    both(hs, lambda h: h.set_action_limits(None, None))
    steps(STEP_PC)
    assert h1.get_step_counter() == h2.get_step_counter() == 10
    h1.close(); h2.close()


def test_filter_switched_on_and_off_on_a_prelaunched_handle(m):
    """(ii) the same through next_device on the handle's own stream with prelaunch 1: with a filter set the pre-launched route is not taken
    (the library falls back to the plain step, and refuses the tuning on a handle that already has a filter); the plain handle's bits"""
    a = MODE["a"]
    hp, h2 = ut.option_handle(m, dict(MODE, tuning={"prelaunch": 1})), ut.option_handle(m, dict(MODE, tuning={"fused_step": 0}))
    hs, x, lim, n = (hp, h2), MODE["x"], ut.LIM_192, 0

    def steps(name1, k=2):
        nonlocal n
        assert hp.rollout_kernel_name().startswith(name1), hp.rollout_kernel_name()
        n += k
        np.testing.assert_array_equal(ut.device_steps(hp, x, k, a), ut.device_steps(h2, x, k, a), err_msg="after %d steps" % n)
        ut.assert_same_state(m, hp, h2, "after %d steps" % n)
    steps(STEP_PC, 3)
    both(hs, lambda h: h.set_sequence_filter(5, 3))
    steps(ROLLOUT_PC)
    both(hs, lambda h: h.set_action_limits(lim["lo"], lim["hi"]))
    steps(ROLLOUT_PC)
    both(hs, lambda h: h.set_sequence_filter(0))
    steps(STEP_PC, 3)
    both(hs, lambda h: h.set_action_limits(None, None))
    steps(STEP_PC)
    assert hp.get_step_counter() == h2.get_step_counter() == 12
    hf = ut.option_handle(m, dict(MODE, filter=(5, 3)))
    with pytest.raises(m.MppiError):
        hf.set_tuning("prelaunch", 1)
    hp.close(); h2.close(); hf.close()


def armable(m):
    h = ut.option_handle(m, MODE)
    try:
        h.set_tuning("armed_us", 100)
        return True
    except Exception:
        return False
    finally:
        h.close()


def test_armed_handle_with_a_filter_steps_like_the_plain_handle(m):
    """(iii) armed launches need the step's shape, which a filter takes away: steps through next equal the plain handle's"""
    if not armable(m):
        pytest.skip("no large-BAR device: MPPI_TUNE_ARMED_US is unsupported here")
    ha, h2 = ut.option_handle(m, dict(MODE, tuning={"armed_us": 20000, "armed_always": 1})), ut.option_handle(m, dict(MODE, tuning={"fused_step": 0}))
    x = MODE["x"]
    for on in (False, True, False):
        both((ha, h2), lambda h: h.set_sequence_filter(5 if on else 0, 3))
        for i in range(3):
            np.testing.assert_array_equal(ha.next(x), h2.next(x))
        ut.assert_same_state(m, ha, h2, "filter %s" % on)  # (reading the state retires the launch armed behind the last call)
    ha.close(); h2.close()
