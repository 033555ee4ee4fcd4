"""The learned-model instance matrix on the GPU: every reachable instance of the learned rollout kernels (tests/learned_matrix_util.py: the lone
and the batched learned point mass, the lone and the batched 13-state NNAUVModel / NNAUVModelSpeed) is launched at K = 160 and its kernel's
edge horizons H = 1, 4, 5, 9 for two fused Philox steps (step counters 0 and 1) and, the lone ones, one step on injected noise, and held to
the fp64 CPU oracle; then at the further shapes of its family (K = 33 / 65 where a tile is owned as two sets of 32, K = 1 / 65 on the one-wave
kernels, K = 64 on the two-tile pipelines). Tests of their own: the pipelines past workgroup 255 (K = 32768 + 65: the roles swap) and at
513 workgroups (K = 65536 + 1: the balance is off by the rule), the tile walkers with one tile more than CUs (K = 64 n_cu + 1), tuning
pc_balance = 0 against the default bit for bit (k_rollout_auv_pc included), and normalizeCost once per kernel family (MODE_COST_ONLY of the
learned kernel, k_cost_normalize, the records from the given costs). That every case is fit to judge a kernel is proven on the CPU by
tests/test_learned_matrix_oracle.py. Needs an MI355X: every test is marked `gpu`.

Bars, each the suite's own (tests/test_parity_gpu.py MLP_VARIANTS / check_mlp_step, tests/batch_mlp_util.py): the noise the step drew within
5e-6 of the oracle's restatement; every sample's cost within 2e-5 relative of the fp64 oracle's and within 4 x max(the fp32 oracle's own
distance on the same noise, 1e-6) (8 x for the split-bf16 kernels); u, DBG_U_UPDATED and the stored sequence within 1e-5 of the fp64 oracle's
(split-bf16: 2e-5); the weights sum to 1 within 1e-5; u is U'[0] exactly; rollout_kernel_name() is the name the restated rule gives; batch
members are also their lone handles bit for bit. normalizeCost: test_normalize_cost_on_the_fused_path's bars against the fp64 oracle's
normalised step — costs rtol 2e-6, u and the sequence 1e-5, weights rtol 2e-4.

The code under test is never its own reference: the fp32 oracle is the measure of what fp32 can do.

Measured on an MI355X over the 92 instances (largest distance per bar): noise 7.2e-7; costs 7.9e-7 relative, 0.20 x their bar relative to the
fp32 oracle (split-bf16: 1.7e-6, 0.22 x); u, U', sequence 6.9e-7 (split-bf16 1.4e-6); sum of the weights 1.4e-7; normalizeCost: costs 2.8e-7
(split-bf16 3.4e-7), u, U', sequence 1.1e-6 (1.4e-6), weights 4.5e-5 (5.1e-5) relative; every bit-for-bit comparison holds, the role swap,
the missing second tile, the balance turned off by the rule and by the tuning included. No case exposed a kernel defect.
"""
import numpy as np
import pytest

import learned_matrix_util as lm
from learned_gpu_util import Lone, Matrix, assert_same_bits, snapshot

pytestmark = pytest.mark.gpu
MX = Matrix()     # the cases on the GPU (tests/learned_gpu_util.py: shared with tests/test_attitude_gpu.py)
RAN = MX.ran      # the names that ran
ENTERED = set()   # the matrix tests that ran
SEEN = MX.seen    # bar -> the largest distance observed
run_lone, run_batch = MX.run_lone, MX.run_batch


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


@pytest.mark.parametrize("group", lm.lone_groups(), ids=lm.group_id)
def test_lone_instances_against_the_oracle(m, group):
    memo = {}
    for c in lm.lone_cases(*group):
        run_lone(m, c, memo)
    ENTERED.add(group)


@pytest.mark.parametrize("group", lm.batch_groups(), ids=lm.group_id)
def test_batched_instances_against_the_oracle_and_their_lone_handles(m, group):
    memo = {}
    for members in lm.batch_cases(*group):
        run_batch(m, members, memo)
    ENTERED.add(group)


@pytest.mark.parametrize("fam,c", lm.normalize_cases(), ids=[f for f, _ in lm.normalize_cases()])
def test_normalize_cost_enters_the_cost_only_pass(m, fam, c):
    """normalizeCost on a learned handle: MODE_COST_ONLY of the family's kernel, k_cost_normalize, then the records from the given costs (the tile
    kernel for the point mass, k_rollout_gen<.., MODE_COSTS_GIVEN> for the 13-state models), against the fp64 oracle's normalised step"""
    assert lm.route(lm.cfg_of(c))[0][0] == lm.kernel_family(fam)
    run_lone(m, c, {})
    ENTERED.add(("normalize", fam))


BIG = lm.big_cases()


@pytest.mark.parametrize("fam,c", BIG, ids=["%s_K%d" % (f, c["K"]) for f, c in BIG])
def test_large_grids_against_the_oracle(m, fam, c):
    """the two-tile pipelines past workgroup 255 (the roles swap with blockIdx.x >> 8) and at 513 workgroups (mppi_two_tile_balance turns
    off above 2 n_cu); the tile walkers at 64 n_cu + 1 rollouts (one workgroup walks a second, ragged tile): every sample's cost and U'"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu == lm.N_CU, "the shapes of this test are an MI355X's (%d compute units), not %d" % (lm.N_CU, n_cu)
    (inst, wgs), = lm.route(lm.cfg_of(c), "next", c["K"], grids=True)
    assert inst[0] == fam
    if fam in lm.PIPELINES:
        assert wgs > 256 and lm.two_tile_balance(lm.create(lm.cfg_of(c)), wgs) == (0 if c["K"] > 65536 else 1)
    else:
        assert wgs == n_cu and lm.tiles(c["K"]) == n_cu + 1
    run_lone(m, c, {})
    ENTERED.add(("big", fam, c["K"]))


BALANCE = lm.balance_cases()


@pytest.mark.parametrize("fam,c", BALANCE, ids=["%s_K%d" % (f, c["K"]) for f, c in BALANCE])
def test_pc_balance_off_is_the_default_bit_for_bit(m, fam, c):
    """tuning pc_balance = 0 (the waves keep the roles of their index, not of their SIMD) against the default: the roles only place waves,
    each tile's arithmetic does not depend on them — costs, u, U', beta, eta and the sequence are equal bit for bit; both runs against the
    oracle"""
    off = dict(c, tuning=dict(c["tuning"], pc_balance=0), id=c["id"] + "_balance0")
    assert lm.create(lm.cfg_of(off))["balance"] == 0 and lm.create(lm.cfg_of(c))["balance"] == 1
    on, un = run_lone(m, c, {}), run_lone(m, off, {})
    for step in range(len(on)):
        assert_same_bits(un[step], on[step], "%s step %d: pc_balance = 0 against the default" % (c["id"], step))
    ENTERED.add(("balance", fam, c["K"]))


@pytest.mark.parametrize("K", [lm.K, 32768 + 65])
def test_pc_balance_off_is_the_default_bit_for_bit_on_the_fossen_pipeline(m, K):
    """the same for k_rollout_auv_pc, whose role assignment is the learned pipelines' (lambda = 2000: the rexrov2 task's costs are 1e4 per
    step, and at lambda = 1 one sample would hold the update)"""
    from batch_util import auv_members, rexrov2
    from mppi_tf_amd.auv import auv_task
    H = lm.EDGE_H if K == lm.K else lm.BIG_H
    t = auv_task(H)
    X, G, U0 = auv_members(1, H, seed=3)
    snaps = []
    for tuning in (None, {"pc_balance": 0}):
        h = m.Handle(k=K, tau=H, s_dim=13, a_dim=6, dt=0.1, lam=2000.0, sigma=t["sigma"], Q=t["Q"], goal=G[0], auv=rexrov2(), seed=77, tuning=tuning)
        assert h.rollout_kernel_name() == "mppi::k_rollout_auv_pc<true>", h.rollout_kernel_name()
        h.set_action_sequence(U0[0])
        snaps.append([snapshot(m, Lone(h), h.next(X[0])) for _ in range(lm.STEPS)])
        h.close()
    for step in range(lm.STEPS):
        assert np.isfinite(snaps[0][step]["costs"]).all() and np.ptp(snaps[0][step]["costs"]) > 0
        assert_same_bits(snaps[1][step], snaps[0][step], "k_rollout_auv_pc K = %d step %d: pc_balance = 0 against the default" % (K, step))


def test_the_names_that_ran_are_the_reachable_set():
    print("\n".join(sorted(RAN)))
    print("%d instances ran; largest distances observed:" % len(RAN))
    for bar in sorted(SEEN):
        print("  %-60s %.3g" % (bar, SEEN[bar]))
    reachable = {lm.fmt(i) for i in lm.reachable_instances()}
    assert RAN <= reachable, sorted(RAN - reachable)
    if ENTERED >= set(lm.lone_groups()) | set(lm.batch_groups()):  # (a run of part of this file has launched part of the set)
        assert RAN == reachable, "reachable, but never launched: %s" % sorted(reachable - RAN)
        assert len(RAN) == 49 + 13 + 22 + 8
