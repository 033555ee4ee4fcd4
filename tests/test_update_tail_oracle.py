"""Every case of the update-tail tests (tests/update_tail_util.py, run on the GPU by tests/test_update_tail_gpu.py) tests what it is meant
to: proven here on the CPU, before a GPU sees it, with the fp64 references alone. The margins are printed per case.

A1: for every record count n and needle record b*, the fp64 combine without b* is at least 100 x U_TOL away and the fp32 evaluation of the
same formula within U_TOL / 4; the plain population moves every column of U' by O(0.1), each column its own way, and weights matter.
A2: every needle of the K = 2^20 + 1 cases is a needle by needle_util's conditions (a), (b), (c); the needles sit in the tiles whose record
slots are the group edges of both fold levels.
B: on the oracle's restated noise, every step of every case has, in every action column of the unclipped update, one entry above the upper
limit, one below the lower one and one strictly inside; the filter moves the sequence; with both options one filtered entry lies outside
the limits; and the three wrong references (option left out, clip indexed c // H, filter before clip) are each 100 bars away.
"""
import numpy as np
import pytest

import needle_util as nu
import update_tail_util as ut


# =============================================================== A1
@pytest.mark.parametrize("n", ut.TREE_N, ids=["n%d" % n for n in ut.TREE_N])
def test_tree_records_test_the_tree(n):
    K, H, a = ut.tree_handle_shape(n)
    assert ut.tree_levels(n) == ut.TREE_LEVELS[n] and ut.tree_fits(n, K), "the handle's scratch must hold the fold"
    assert (K + 63) // 64 >= n or n <= ut.kOnePass
    U = ut.tree_U(H, a)
    assert np.abs(U).min() > 0.1
    # the plain population
    rec = ut.tree_records(n, H * a)
    lam = float(nu.F32(ut.TREE_LAM))
    assert rec[:, 0].min() >= 0 and rec[:, 0].max() < 2 * lam and rec[:, 1].min() >= 1 and rec[:, 1].max() <= 64 and np.abs(rec[:, 2:]).max() <= 1
    beta, eta, Uu = ut.tree_reference(rec, U)
    cond = np.abs(ut.tree_reference(rec, U, dtype=np.float32)[2].astype(np.float64) - Uu).max()
    flat = (rec[:, 1:2].astype(np.float64) * rec[:, 2:]).sum(axis=0) / rec[:, 1].astype(np.float64).sum()  # every r_b taken for 1
    d = (Uu - U).ravel()
    print("n = %d plain: beta %.6g eta %.6g |U' - U| per column %s, unweighted off by %.3g, fp32 off by %.3g" % (n, beta, eta, np.abs(d), np.abs(flat - d).max(), cond))
    assert cond <= ut.TREE_COND_MAX
    if n > 1:
        assert np.abs(d).min() >= 1000 * nu.U_TOL, "a column of the plain population hardly moves"
        assert np.abs(flat - d).max() >= 100 * nu.U_TOL, "the weights do not matter"
        if H * a > 1:
            assert np.abs(d[:, None] - d[None, :])[~np.eye(H * a, dtype=bool)].min() >= 100 * nu.U_TOL, "two columns move alike: a wrong column would pass"
    # the needle populations
    want = {b for b in (0, n - 1, 15, 16, 255, 256, 4095, 4096) if b < n} if n > 1 else set()
    assert set(ut.tree_needles(n)) == want
    if ut.tree_levels(n) >= 1:  # from n = 16385 on the last group holds one record at every level
        g = n
        while g > ut.kOnePass:
            assert n < 16385 or g % ut.kGroup == 1
            g = (g + ut.kGroup - 1) // ut.kGroup
    for b in ut.tree_needles(n):
        rec = ut.tree_records(n, H * a, b)
        others = np.delete(rec[:, 0], b)
        assert rec[b, 0] == 0 and rec[b, 1] == 1 and np.abs(rec[b, 2:]).min() == 1 and others.min() >= 14 * lam
        loo, cond, w = ut.assert_tree_case(n, b, rec, U)
        print("n = %d b* = %d: weight %.9f, without it U' moves by %.3g, fp32 off by %.3g" % (n, b, w, loo, cond))
        assert w >= nu.W_MIN


def test_shard_finish_rule_refuses_what_the_gpu_test_expects():
    """the small handle of the refusal test (K = 192: 128 record slots, scratch for 8 folded records) holds 1024 records and no fold"""
    assert ut.tree_fits(1024, 192) and not ut.tree_fits(1025, 192) and not ut.tree_fits(20000, 192)
    assert all(ut.tree_fits(n, ut.tree_handle_shape(n)[0]) for n in ut.TREE_N)


# =============================================================== A2
def test_two_level_needles_sit_on_the_group_edges():
    nb, nbp = ut.K20_NB, ut.K20_NBP
    assert (nb, nbp) == (16385, 16512) and ut.tree_levels(nb) == 2 and ut.tree_levels(2 ** 20 // 64) == 1
    record_slot = lambda b: (b & 7) * (nbp >> 3) + (b >> 3)  # mppi_device.hip.h
    tiles = [ut.slot_tile(s, nbp) for s in ut.K20_SLOTS]
    assert all(b < nb for b in tiles) and [record_slot(b) for b in tiles] == ut.K20_SLOTS
    assert max(record_slot(b) for b in range(nb)) == 16495, "16495 is the highest slot a tile owns"
    assert [k // 64 for k in ut.K20_KS[:-1]] == tiles and ut.K20_KS[-1] == ut.K20 - 1 and ut.K20_KS[-1] // 64 == nb - 1
    assert sorted(k for c in ut.TWO_LEVEL[:3] for k in c["ks"]) == sorted(ut.K20_KS)
    assert ut.TWO_LEVEL[3]["normalize"] and ut.TWO_LEVEL[3]["ks"] == [ut.K20_KS[0], ut.K20_KS[2], ut.K20 - 1]  # first tile, slot 256, last sample


@pytest.mark.parametrize("case", ut.TWO_LEVEL, ids=nu.ids(ut.TWO_LEVEL))
def test_two_level_case_is_a_needle(case):
    p32, p64 = nu.problems(case)
    eps, x, gaps = nu.oracle_noise(case), nu.goal_of(case), []
    for k in case["ks"]:
        ref = nu.reference(case, p32, p64, x, eps, k)
        c = np.sort(ref["c64"])
        gaps.append((c[1] - c[0]) / ((c[-1] - c[0]) if case["normalize"] else 1.0))
        print("%s k* = %d: w_ref %.9f, leave-one-out distance %.3g, fp32 oracle off by %.3g, gap %.4g" % (case["id"], k, ref["w"], ref["loo"], ref["cond"], gaps[-1]))
        nu.assert_is_needle(case, k, ref)
        assert ref["c32"][k] == 0.0 and ref["c64"][k] == 0.0 and ref["c32"].min() == 0.0
    ninth = min(gaps) / 9
    assert 0.85 * ninth <= case["lam"] <= 1.15 * ninth, "lambda %g is not about a ninth of the smallest gap %g" % (case["lam"], min(gaps))


# =============================================================== B
def test_option_cases_cover_the_paths():
    cases = ut.OPTION_CASES
    assert len(set(nu.ids(cases))) == len(cases)
    for c in cases:
        assert c["limits"] or c["filter"]
        if c["limits"]:
            assert len(c["lo"]) == len(c["hi"]) == c["a"] and all(l < h for l, h in zip(c["lo"], c["hi"]))
        if c["filter"]:
            assert c["filter"][0] % 2 == 1 and c["filter"][1] < c["filter"][0] <= c["H"]
    assert any(c["filter"] and c["filter"][0] == c["H"] for c in cases), "a window equal to H: every row an edge row"
    assert {c["path"] for c in cases} == {"lone", "shards3", "p2p2", "pre"} and {c["model"] for c in cases} == {"pm", "mlp", "auv"}


@pytest.mark.parametrize("case", ut.OPTION_CASES, ids=nu.ids(ut.OPTION_CASES))
def test_option_case_tests_its_options(case):
    worst = {}
    for s, (Uraw, margins) in enumerate(ut.cpu_steps(case)):
        if margins is None:
            continue
        print("%s step %d: %s" % (case["id"], s, ", ".join("%s %.0f" % kv for kv in margins.items())))
        for k, v in margins.items():
            worst[k] = min(worst.get(k, np.inf), v)
    print("%s, least margins in bars: %s" % (case["id"], ", ".join("%s %.0f" % kv for kv in worst.items())))
    assert worst and min(worst.values()) >= ut.MARGIN


def test_filter_bar_is_the_rounding_of_an_fp32_sum():
    """the bar of the stored sequence: the fp32 evaluation of the filter (weights and inputs rounded to fp32, fp32 accumulation) stays
    within it on every case's own first update"""
    for case in [c for c in ut.OPTION_CASES if c["filter"]]:
        H, (w, p) = case["H"], case["filter"]
        rows, start = ut.savgol_rows(H, w, p)
        np.testing.assert_allclose(rows @ np.eye(w), rows)
        Uu, seq = ut.option_reference(case, ut.cpu_steps(dict(case, counts=(1,)), check=False)[0][0])
        sh = ut.shifted(Uu.astype(np.float32))
        got = np.zeros_like(sh)
        for t in range(H):
            acc = np.zeros(case["a"], np.float32)
            for i in range(w):
                acc = acc + rows[t, i].astype(np.float32) * sh[start[t] + i]
            got[t] = acc
        d, bar = np.abs(got - ut.savgol(sh, w, p)).max(), ut.filter_bar(H, w, p, Uu)
        print("%s: fp32 filter off by %.3g, bar %.3g" % (case["id"], d, bar))
        assert d <= bar
