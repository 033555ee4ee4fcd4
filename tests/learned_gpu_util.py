"""What the GPU files of the instance matrices share (test_learned_matrix_gpu.py, test_attitude_gpu.py): one case of learned_matrix_util on a lone
handle or as a member of a batch, every step against the oracle at the suite's bars (the bars and what they mean: test_learned_matrix_gpu.py's
docstring), and the record of what ran. A plain module: `m` is the mppi_tf_amd package each test file's fixture gives."""
import numpy as np

import learned_matrix_util as lm

NOISE_TOL = 5e-6
COST_BAR = 2e-5


class Lone:
    def __init__(self, h):
        self.h = h

    def dbg(self, what):
        return self.h.debug_get(what)

    def sequence(self):
        return self.h.get_action_sequence()


class Member:
    def __init__(self, hb, i):
        self.hb, self.i = hb, i

    def dbg(self, what):
        return self.hb.debug_get(self.i, what)

    def sequence(self):
        return self.hb.get_action_sequences()[self.i]


def snapshot(m, view, u):
    """what one step left: the bits a batch member and its lone handle (the balanced and the unbalanced pipeline) must share"""
    return dict(u=np.array(u), costs=view.dbg(m.DBG_COSTS), beta=float(view.dbg(m.DBG_BETA)), eta=float(view.dbg(m.DBG_ETA)),
                Uupd=view.dbg(m.DBG_U_UPDATED), seq=view.sequence())


def assert_same_bits(got, want, tag):
    for key in ("u", "costs", "Uupd", "seq"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (tag, key))
    assert got["beta"] == want["beta"] and got["eta"] == want["eta"], (tag, got["beta"], want["beta"], got["eta"], want["eta"])


class Matrix:
    """the runs of one test file: the names that ran, the largest distance observed per bar"""

    def __init__(self):
        self.ran, self.seen = set(), {}

    def see(self, bar, value):
        self.seen[bar] = max(self.seen.get(bar, 0.0), float(value))

    def check_step(self, m, view, c, mk, p32, p64, U_in, eps, snap, tag):
        """one step of case c (it read the sequence U_in and the noise eps) against the oracle on that noise; every figure is printed before
        it is asserted"""
        x, nrm, kind = mk["x"], c["normalize"], "split-bf16 " if lm.split_bf16(c) else ""
        u64, Us64, c64 = p64.next_with_noise(x, U_in, eps, normalize=nrm)
        _, _, c32 = p32.next_with_noise(x, U_in, eps, normalize=nrm)
        c64 = np.asarray(c64, np.float64)
        rel = float((np.abs(snap["costs"].astype(np.float64) - c64) / np.abs(c64)).max())
        rel32 = float((np.abs(np.asarray(c32, np.float64) - c64) / np.abs(c64)).max())
        Uupd64 = lm.updated(u64, Us64)
        d = max(np.abs(snap["u"] - u64).max(), np.abs(snap["Uupd"] - Uupd64).max(), np.abs(snap["seq"] - Us64).max())
        w = view.dbg(m.DBG_WEIGHTS).astype(np.float64)
        print("%s: costs %.3g relative (fp32 oracle %.3g); u, U', sequence %.3g; sum of the weights - 1 %.3g" % (tag, rel, rel32, d, w.sum() - 1.0))
        if nrm:
            self.see("normalize: %scosts (rtol 2e-6)" % kind, rel)
            self.see("normalize: %su, U', sequence (1e-5)" % kind, d)
            cn = (c64 - c64.min()) / (c64.max() - c64.min())
            w_ref = np.exp(-cn / mk["lam"])
            w_ref /= w_ref.sum()
            self.see("normalize: %sweights (rtol 2e-4)" % kind, (np.abs(w - w_ref) / np.maximum(w_ref, 1e-5)).max())
            np.testing.assert_allclose(snap["costs"], c64, rtol=2e-6, err_msg=tag + ": costs")
            np.testing.assert_allclose(w, w_ref, rtol=2e-4, atol=1e-9, err_msg=tag + ": weights")
            bar = 1e-5
        else:
            factor, bar = lm.cost_factor(c), lm.u_bar(c)
            self.see("%scosts (2e-5 relative)" % kind, rel)
            self.see("%scosts / (%d x max(fp32 oracle, 1e-6))" % (kind, factor), rel / (factor * max(rel32, 1e-6)))
            self.see("%su, U', sequence (%.0e)" % (kind, bar), d)
            assert rel <= COST_BAR, "%s: costs %.3g relative from the fp64 oracle's" % (tag, rel)
            assert rel <= factor * max(rel32, 1e-6), "%s: costs %.3g relative, the fp32 oracle's %.3g" % (tag, rel, rel32)
        np.testing.assert_allclose(snap["u"], u64, rtol=0, atol=bar, err_msg=tag + ": u")
        np.testing.assert_allclose(snap["Uupd"], Uupd64, rtol=0, atol=bar, err_msg=tag + ": U'")
        np.testing.assert_allclose(snap["seq"], Us64, rtol=0, atol=bar, err_msg=tag + ": the stored sequence")
        self.see("sum of the weights (1e-5)", abs(w.sum() - 1.0))
        assert abs(w.sum() - 1.0) <= 1e-5, (tag, w.sum())
        np.testing.assert_array_equal(snap["u"], snap["Uupd"][0], err_msg=tag + ": u is U'[0]")

    def drawn_noise(self, m, view, c, step, tag):
        eps = view.dbg(m.DBG_NOISE)
        d = np.abs(eps - lm.noise(c, step)).max()
        self.see("noise (5e-6)", d)
        assert d <= NOISE_TOL, "%s: the noise is %.3g from the oracle's restatement" % (tag, d)
        return eps

    def run_lone(self, m, c, memo, injected=True, n_cu=lm.N_CU):
        """case c on a lone handle: the fused Philox steps and (injected) one step on injected noise, each against the oracle; -> the steps'
        snapshots (memo: by case id, within one test)"""
        if c["id"] in memo:
            return memo[c["id"]]
        mk, cfg = lm.make_case(c), lm.cfg_of(c)
        h = m.Handle(**mk["handle"])
        name = h.rollout_kernel_name()
        assert name == lm.expected_name(cfg), "%s runs %s, not %s" % (c["id"], name, lm.expected_name(cfg))
        p32, p64 = lm.problems(mk)
        h.set_action_sequence(mk["U"])
        U_in, snaps = mk["U"], []
        for step, call in enumerate(lm.calls(c) if injected else lm.calls(c)[:lm.STEPS]):
            tag = "%s step %d (%s)" % (c["id"], step, call)
            if call == "next":
                u = h.next(mk["x"])
                snaps.append(snapshot(m, Lone(h), u))
                eps = self.drawn_noise(m, Lone(h), c, step, tag)
            else:
                eps = lm.noise(c, lm.INJECTED_STEP)
                u = h.next_with_noise(mk["x"], eps)
                snaps.append(snapshot(m, Lone(h), u))
            self.check_step(m, Lone(h), c, mk, p32, p64, U_in, eps, snaps[-1], tag)
            U_in = snaps[-1]["seq"]
            self.ran.update(lm.fmt(i) for i in lm.route(cfg, call, c["K"], n_cu) if i[0] != "tile")
        assert h.get_step_counter() == len(snaps)
        h.close()
        memo[c["id"]] = snaps
        return snaps

    def run_batch(self, m, members, memo):
        """B members with their own network, seed, goal, lambda and Sigma scale in one launch: each against the oracle, and its lone handle
        bit for bit"""
        c0, mks = members[0], [lm.make_case(c) for c in members]
        model = {"pm": "mlp", "nnauv": "nnauv", "nnspeed": "nnauv_speed"}[c0["kind"]]
        hb = m.BatchHandle.learned(lm.B, [lm.net_of(c) for c in members], model, a_dim=c0["a"], k=c0["K"], tau=c0["H"], dt=0.1,
                                   seeds=[c["seed"] for c in members], lams=[mk["lam"] for mk in mks], sigmas=[lm.sigma_of(c) for c in members],
                                   Q=lm.q_of(c0), goals=np.stack([lm.goal_of(c) for c in members]))
        cfg = lm.batch_cfg(members)
        name = hb.rollout_kernel_name()
        assert name == lm.expected_name(cfg), "the batch of %s runs %s, not %s" % (c0["id"], name, lm.expected_name(cfg))
        lone = [self.run_lone(m, c, memo, injected=False) for c in members]
        hb.set_action_sequences(np.stack([mk["U"] for mk in mks]))
        oracles = [lm.problems(mk) for mk in mks]
        U_in = [mk["U"] for mk in mks]
        for step in range(lm.STEPS):
            u = hb.next(np.stack([mk["x"] for mk in mks]))
            for i, c in enumerate(members):
                tag = "batch of %s member %d step %d" % (c0["id"], i, step)
                snap = snapshot(m, Member(hb, i), u[i])
                eps = self.drawn_noise(m, Member(hb, i), c, step, tag)
                self.check_step(m, Member(hb, i), c, mks[i], oracles[i][0], oracles[i][1], U_in[i], eps, snap, tag)
                assert_same_bits(snap, lone[i][step], tag + " against its lone handle")
                U_in[i] = snap["seq"]
        hb.close()
        self.ran.add(name)
