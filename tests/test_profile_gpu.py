"""mppi_profile_begin / mppi_profile_end on every way a control step is enqueued. Needs an MI355X: every test is marked `gpu`.

Profiling changes how a step is launched (the dominant kernel goes out with its own begin / end events, the tile kernel is bracketed by
recorded ones, a one-launch step records an empty finish interval) and must change nothing else. Per case two identically configured
controllers: A runs unprofiled; B calls profile_begin(2), runs three steps, calls profile_end() and goes on. Then
  * profile_end reports exactly 2 steps (the cap holds; the third step is not recorded), rollout time > 0 and finish time >= 0;
  * every step's u, the action sequence, MPPI_DBG_COSTS and MPPI_DBG_WEIGHTS are the same bits on A and B;
  * profile_end without steps gives zeros, and a second profile_begin counts from zero again;
  * on a sharded controller a step is recorded by mppi_shard_finish: the first half alone records nothing.
Small shapes: K = 128, H = 8, a = 2 unless a case says otherwise."""
import numpy as np
import pytest

from batch_util import rexrov2
from test_parity_gpu import make_mlp, make_mlp_pair

pytestmark = pytest.mark.gpu
F32 = np.float32
STEPS = 5  # three under profile_begin(2), a fourth after profile_end, a fifth under the second profile_begin


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def pm(K=128, H=8, a=2, **kw):
    """the keywords of a point-mass Handle / BatchHandle"""
    s = 2 * a
    return dict(dict(k=K, tau=H, s_dim=s, a_dim=a, dt=0.1, lam=0.7, sigma=0.25 * np.eye(a), goal=[1, 0, .5, 0, .75, 0][:s], Q=np.ones(s), seed=7), **kw)


X_PM = np.array([0.2, 0.1, -0.3, 0.0], F32)


class Rig:
    """One controller under test: its handles (B's are all profiled), step(i) runs control step i, controls() gives the u of every step so
    far, state() the sequences and the (costs, weights) of the last step. every_step: state() may be read between any two steps."""
    every_step = True

    def __init__(self, m, *handles):
        self.m, self.hs, self.u = m, list(handles), []

    def controls(self):
        return np.asarray(self.u)

    def state(self):
        m = self.m
        return [(h.get_action_sequence(), h.debug_get(m.DBG_COSTS), h.debug_get(m.DBG_WEIGHTS)) for h in self.hs]

    def close(self):
        for h in self.hs:
            h.close()


class Host(Rig):
    """mppi_next, or mppi_next_with_noise on noise that depends on the step alone"""

    def __init__(self, m, x, noise=False, handle=None, **kw):
        super().__init__(m, handle or m.Handle(**kw))
        self.x, self.noise = x, noise

    def step(self, i):
        h = self.hs[0]
        if self.noise:
            eps = (0.5 * np.random.default_rng(40 + i).standard_normal((h.k_local, h.tau, h.a))).astype(F32)
            self.u.append(h.next_with_noise(self.x, eps))
        else:
            self.u.append(h.next(self.x))


class Prelaunched(Rig):
    """mppi_next_device on the handle's own stream with MPPI_TUNE_PRELAUNCH: steps stay in flight on the handle's two streams, each with a
    u slot of its own, until something else is asked of the handle"""
    every_step = False

    def __init__(self, m, x, **kw):
        import torch
        super().__init__(m, m.Handle(tuning={"prelaunch": 1}, **kw))
        self.xd = torch.tensor(x, device="cuda")
        self.ud = torch.zeros(STEPS, kw["a_dim"], device="cuda")
        torch.cuda.synchronize()
        self.n = 0

    def step(self, i):
        self.hs[0].next_device(self.xd.data_ptr(), self.ud[i].data_ptr(), None)
        self.n = i + 1

    def controls(self):
        import torch
        self.hs[0].synchronize()
        torch.cuda.synchronize()
        return self.ud[:self.n].cpu().numpy()


class Batch(Rig):
    def __init__(self, m, X, **kw):
        super().__init__(m, m.BatchHandle(n=len(X), **kw))
        self.X = X

    def step(self, i):
        self.u.append(self.hs[0].next(self.X))

    def state(self):
        m, hb = self.m, self.hs[0]
        return [(hb.get_action_sequences(),) + tuple(hb.debug_get(i, what) for i in range(hb.n) for what in (m.DBG_COSTS, m.DBG_WEIGHTS))]


class Shards(Rig):
    """two shards of one controller stepped in one process: the first half on each, the records side by side, mppi_shard_finish on each"""

    def __init__(self, m, x, **kw):
        import torch
        super().__init__(m, *[m.Handle(shard_rank=g, shard_count=2, **kw) for g in range(2)])
        self.normalize = bool(kw.get("normalize_cost"))
        n = self.hs[0].record_size
        self.xd = torch.tensor(x, device="cuda")
        self.recs = torch.zeros(2, n, device="cuda")
        self.rng = torch.zeros(2, 2, device="cuda")
        self.ud = torch.zeros(2, kw["a_dim"], device="cuda")
        torch.cuda.synchronize()

    def first_half(self):
        import torch
        if self.normalize:
            for g, h in enumerate(self.hs):
                h.shard_cost_range(self.xd.data_ptr(), self.rng[g].data_ptr())
                h.synchronize()
            agreed = self.rng.max(dim=0).values.contiguous()  # the all-reduce(MAX) of the {-min, max} pairs
            torch.cuda.synchronize()
        for g, h in enumerate(self.hs):
            if self.normalize:
                h.shard_partial_normalized(self.xd.data_ptr(), agreed.data_ptr(), self.recs[g].data_ptr())
            else:
                h.shard_partial(self.xd.data_ptr(), self.recs[g].data_ptr())
            h.synchronize()

    def step(self, i):
        self.first_half()
        for g, h in enumerate(self.hs):
            h.shard_finish(self.recs.data_ptr(), 2, self.ud[g].data_ptr())
            h.synchronize()
        self.u.append(self.ud.cpu().numpy().copy())


def auv_kw():
    from mppi_tf_amd.auv import auv_task
    t = auv_task(4)
    return dict(k=128, tau=4, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=t["sigma"], Q=t["Q"], auv=rexrov2(), seed=7)


X_AUV = np.array([0.3, -0.2, 0.5, 1, 0, 0, 0, 0.1, 0, -0.1, 0, 0.05, 0], F32)
X_B2 = np.array([[0.2, 0.1, -0.3, 0.0], [-0.4, 0.0, 0.1, 0.2]], F32)


def mlp_rig(m):
    """a small learned model (Dense(32) x 3, the reference's own network shape)"""
    return Host(m, X_PM, handle=make_mlp_pair(m, 128, 8, 2, make_mlp(4, 2, seed=4, hid=32, n_hidden=3), lam=0.7, seed=7)[0])


# id -> (a substring of the rollout kernel's name, or None where the case's steps are not the handle's plain Philox step; the rig's factory)
CASES = {
    "fused": ("k_step_pc<", lambda m: Host(m, X_PM, **pm())),
    "two_launches": ("k_rollout_pc<", lambda m: Host(m, X_PM, tuning={"fused_step": 0}, **pm())),
    "normalize_two_pc_passes": ("k_rollout_pc<", lambda m: Host(m, X_PM, **pm(K=192, normalize_cost=True))),
    "tile": ("k_rollout_tile<", lambda m: Host(m, X_PM, tuning={"force_tile_kernel": 1}, **pm())),
    "tile_normalize_three_launches": ("k_rollout_tile<", lambda m: Host(m, X_PM, tuning={"force_tile_kernel": 1}, **pm(normalize_cost=True))),
    "next_with_noise": (None, lambda m: Host(m, X_PM, noise=True, **pm())),
    "prelaunch": ("k_step_pc<", lambda m: Prelaunched(m, X_PM, **pm())),
    "learned_model": ("k_rollout_mlp", mlp_rig),
    "fossen_auv": ("k_rollout_auv_pc<", lambda m: Host(m, X_AUV, **auv_kw())),
    "batch_of_two": ("k_rollout_pc_batch<", lambda m: Batch(m, X_B2, **pm())),
    "two_shards": ("k_rollout_pc<", lambda m: Shards(m, X_PM, **pm())),
    "two_shards_normalize": ("k_rollout_pc<", lambda m: Shards(m, X_PM, **pm(normalize_cost=True))),
}


def assert_same(A, B, tag):
    np.testing.assert_array_equal(B.controls(), A.controls(), err_msg="u, " + tag)
    for g, (sa, sb) in enumerate(zip(A.state(), B.state())):
        for j, (va, vb) in enumerate(zip(sa, sb)):
            np.testing.assert_array_equal(vb, va, err_msg="handle %d, item %d (sequence, then costs and weights), %s" % (g, j, tag))


@pytest.mark.parametrize("case", list(CASES))
def test_profiled_steps_are_the_unprofiled_steps(m, case):
    expect, make = CASES[case]
    A, B = make(m), make(m)
    try:
        if expect:
            for h in B.hs:
                assert expect in h.rollout_kernel_name(), h.rollout_kernel_name()
        for h in B.hs:
            h.profile_begin(2)
        for i in range(3):
            A.step(i)
            B.step(i)
            if B.every_step:
                assert_same(A, B, "after step %d" % (i + 1))
        for h in B.hs:
            r, f, n = h.profile_end()
            print("%s: rollout %.3f us, finish %.3f us, %d steps" % (case, r * 1e3, f * 1e3, n))
            assert n == 2, "the cap of 2 steps: %d recorded" % n
            assert r > 0.0 and f >= 0.0, (r, f)
        assert_same(A, B, "after three steps, two of them profiled")
        A.step(3)
        B.step(3)
        assert_same(A, B, "after the step behind profile_end")
        # no step between begin and end: zeros (a sharded controller's first half alone is no step: mppi_shard_finish records it)
        for h in B.hs:
            h.profile_begin(2)
        if isinstance(B, Shards):
            B.first_half()
        for h in B.hs:
            assert h.profile_end() == (0.0, 0.0, 0)
        # a second profile counts from zero
        for h in B.hs:
            h.profile_begin(3)
        A.step(4)
        B.step(4)
        for h in B.hs:
            r, f, n = h.profile_end()
            assert n == 1 and r > 0.0 and f >= 0.0, (r, f, n)
        assert_same(A, B, "after the step of the second profile")
    finally:
        A.close()
        B.close()
