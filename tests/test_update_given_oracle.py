"""Every designed input of the update-on-given-costs tests (tests/update_given_util.py, run on the GPU by tests/test_update_given_gpu.py)
tests what it is meant to: proven here on the CPU oracle, before a GPU sees it, with needle_util's constants (no new bars).

For every case of every shape: orc.update in fp32 is within COND_MAX of orc.update(dtype=float64) on U' and within ETA_RTOL / 4 on eta,
so what the GPU is held to is the kernel's error and not the case's conditioning. A needle's fp64 weight is at least W_MIN and leaving
it out moves the fp64 U' by at least LOO_MIN. stairs has a whole tile whose fp64 weights lie below 1e-38 with a finite reference, and no
exp or w of it within a factor 2 of the 1e-30 line that decides which samples are compared. The slots 0, 255, 256, 511, 512, 767, 768
and nbp - 1 are each the home of a needle at every j where they exist, and the reached record counts are 128 .. 1024 in steps of 128
plus one fold.

Measured here (fp32 oracle against fp64, over the 257 cases): U' within 1.22e-7 on the H = 4 shapes and 9.46e-7 at H = 40 (|U| up to 20:
half an ulp), eta within 5.62e-8 relative; every needle's leave-one-out distance is at least 0.998. The fp32 oracle's own arg is within
1.18e-7 relative (0.661 of arg_bar) and its exp within 5.24e-6 (0.57 of exp_rbar): the bars the GPU is held to leave a correct fp32
evaluation room, and not much.
"""
import numpy as np
import pytest

import needle_util as nu
import update_given_util as ug

WORST = {}


def test_shapes_reach_every_record_count_and_every_named_slot():
    assert sorted({s["nbp"] for s in ug.MATRIX}) == list(range(128, 1025, 128))
    assert [s["nbp"] for s in ug.SHAPES if s["nbp"] > 1024] == [1152] and ug.FOLD["nb"] == 1025
    assert ug.WIDE["nbp"] == ug.AUV["nbp"] == 384 and ug.WIDE["H"] * ug.WIDE["a"] == 160 and (ug.AUV["H"], ug.AUV["a"]) == (3, 6)
    for j in ug.J_ALL:
        full, ragged = [s for s in ug.MATRIX if s["j"] == j]
        assert not full["ragged"] and ragged["ragged"] and full["nbp"] == ragged["nbp"] == 128 * j
        assert full["K"] == 64 * full["nbp"] and full["nb"] == full["nbp"], "full: every slot a real tile"
        assert ragged["nb"] == 128 * (j - 1) + 1 and ragged["K"] == 64 * (ragged["nb"] - 1) + 1, "ragged: one sample in the first tile of a new block"
        hit = {slot for s in (full, ragged) for _, slot in ug.needles(s)}
        want = {s for s in ug.SLOT_TARGETS + (128 * j - 1,) if s < 128 * j}
        assert want <= hit, "j = %d: no needle in slot(s) %s" % (j, sorted(want - hit))
        for s in (full, ragged):
            ks = [k for k, _ in ug.needles(s)]
            assert set(ks) >= {k for k in (0, 63, 64, s["K"] - 1) if k < s["K"]} or s["K"] == 1
            assert all(0 <= k < s["K"] for k in ks) and all(ug.record_slot(k // 64, s["nbp"]) == slot for k, slot in ug.needles(s))
        assert (ragged["K"] - 1) // 64 == ragged["nb"] - 1 and (ragged["K"] - 1) % 64 == 0, "the last sample is alone in its tile"
    assert {s["a"] for s in ug.MATRIX if s["ragged"]} == {s["a"] for s in ug.MATRIX if not s["ragged"]} == {1, 2, 3, 4}
    # record_slot and its inverse, and that pads lie between real records wherever a block is not full
    for nbp in (128, 384, 1152):
        assert sorted(ug.record_slot(b, nbp) for b in range(nbp)) == list(range(nbp))
        assert all(ug.slot_tile(ug.record_slot(b, nbp), nbp) == b for b in range(nbp))
    owned = sorted(ug.record_slot(b, 384) for b in range(257))
    assert owned[-1] > 257 and len(set(range(owned[-1])) - set(owned)) > 0


def test_every_shape_runs_every_family_it_must():
    for s in ug.SHAPES:
        cs = ug.cases(s)
        assert len(set(cs)) == len(cs) and ("spread", 1.0, None) in cs
        assert [c[2] for c in cs if c[0] == "needle" and c[1] == 1.0] == [k for k, _ in ug.needles(s)]
        if s["more"]:
            assert s["j"] in ug.J_MORE
            for lam in ug.LAMS:
                assert ("ties", lam, None) in cs and ("spread", lam, None) in cs
                assert (("stairs", lam, None) in cs) == (s["nb"] >= ug.STAIRS_MIN_NB)
                assert s["K"] == 1 or sum(c[0] == "needle" and c[1] == lam for c in cs) >= 2
    assert {s["j"] for s in ug.MATRIX if s["more"]} == set(ug.J_MORE)
    assert [s["id"] for s in ug.SHAPES if s["nb"] < ug.STAIRS_MIN_NB or s["K"] == 1] == ["j1_ragged_a3"], "only K = 1 goes without stairs and needles"


@pytest.mark.parametrize("sh", ug.SHAPES, ids=ug.SHAPE_IDS)
def test_case_tests_the_update(sh):
    for case in ug.cases(sh):
        family, lam, k = case
        tag = "%s %s" % (sh["id"], ug.case_id(case))
        cost, eps, U, lam32 = ug.inputs(sh, case)
        assert cost.dtype == eps.dtype == U.dtype == np.float32 and np.isfinite(cost).all() and np.isfinite(eps).all()
        r64, r32 = ug.reference(cost, eps, U, lam32), ug.reference(cost, eps, U, lam32, dtype=np.float32)
        assert all(np.isfinite(r64[key]).all() for key in r64), tag
        cond = np.abs(r32["Unew"] - r64["Unew"]).max()
        eta = abs(float(r32["nabla"]) - r64["nabla"]) / r64["nabla"]
        d = ug.distances(r32, r64)
        ug.worse(WORST, d)
        print("%s: fp32 oracle off by %.3g on U', %.3g on eta, arg %.2f and exp %.2f of their bars" % (tag, cond, eta, d["arg_of_bar"], d["exp_of_bar"]))
        assert cond <= nu.COND_MAX, "%s: the fp32 oracle's U' is %.3g from the fp64 one" % (tag, cond)
        assert eta <= nu.ETA_RTOL / 4, "%s: the fp32 oracle's eta is %.3g from the fp64 one" % (tag, eta)
        assert r64["beta"] == cost.min()
        if family == "needle":
            assert cost[k] == 0 and np.delete(cost, k).min() >= 14 * lam32 and np.abs(eps[k]).min() == 1 == np.abs(eps[k]).max()
            loo = np.abs(ug.reference(cost, eps, U, lam32, without=k)["Unew"] - r64["Unew"]).max()
            print("%s: weight %.9f, without it U' moves by %.3g" % (tag, r64["w"][k], loo))
            WORST["loo"] = min(WORST.get("loo", np.inf), loo)
            assert r64["w"][k] >= nu.W_MIN, "%s: the needle weighs %.6f" % (tag, r64["w"][k])
            assert loo >= nu.LOO_MIN, "%s: losing the needle moves U' by %.3g" % (tag, loo)
        if family == "stairs":
            w = np.concatenate([r64["w"], np.zeros(-sh["K"] % 64)]).reshape(-1, 64)
            assert (w.max(axis=1) < 1e-38).any(), "%s: no whole tile underflows" % tag
            for key in ("exp", "w"):
                v = r64[key]
                assert not ((v > ug.TINY / 2) & (v < ug.TINY * 2)).any(), "%s: an %s on the line between compared and not" % (tag, key)
                assert (v < ug.TINY).any() and (v >= ug.TINY).any()
        else:
            assert (r64["exp"] >= ug.TINY).all() and (r64["w"] >= ug.TINY).all(), "%s: only stairs may have samples below %g" % (tag, ug.TINY)
        assert d["arg_of_bar"] <= 1 and d["exp_of_bar"] <= 1, "%s: the fp32 oracle itself misses the derived bars" % tag
    print("worst so far over %d cases: %s" % (WORST["n"], ", ".join("%s %.3g" % kv for kv in sorted(WORST.items()) if kv[0] != "n")))
