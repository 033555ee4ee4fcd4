"""Batched controllers against the alternatives a user has without them, at one shape, in one process:
  (a) one BatchHandle of B members: one batched step = the rollout and the finish of every member, two launches;
  (b) B plain Handles, each on its own stream, stepped round-robin from one host thread (the tools/two_controllers.py pattern);
  (c) one plain Handle alone.
Each figure is a host clock around `steps` pipelined next_device steps (rounds of B steps for (b)) that end in a synchronise; the three
alternate, `reps` times, and the median is printed: us per batched step (per round for (b)), us per controller step, rollouts/s.
--model auv: the Fossen AUV model at the reference's task (mppi_tf_amd.auv.auv_task: rexrov2, rk2, Sigma = 1500 I, the static goal),
with the x0 of that task for every controller.
--sweep: a parameter sweep against a uniform batch of the same shape (B = 16: the point mass at K=4096 H=64 a=2 and K=3000 H=50 a=3, the
AUV at K=4096 H=40). In the sweep batch every member has its own lambda (log-spaced 0.1 to 10), Sigma scale (0.5 to 2) and Q scale (0.5
to 2); the uniform batch shares the configuration. The two alternate as above. --only uniform times the uniform batch alone (through
BatchHandle's shared keywords only, so the tool also runs on a package without per-member parameters).
    tools/time_batch.py [--model pm|auv] [--steps N] [--reps R] [--quick] [--only batch|streams|single] [--shape B,K,H] [--dry-run]
    tools/time_batch.py --sweep [--only sweep|uniform] [--steps N] [--reps R] [--dry-run]
--model nnauv|nnspeed [--hid 16|32 --layers 1..3]: the learned 13-state models with ONE NETWORK PER MEMBER (BatchHandle.learned) at K = 1024,
H = 32, B in {8, 32, 128}: the batch; B lone DEFAULT handles stepped one after another on one stream (what a user does without the batch);
the same B handles on B streams; and the batch's rollout kernel time (its own dispatch timestamps) with B distinct networks against B
members sharing ONE network. --only batch|shared|serial|streams times one alone (a counter or kernel-trace run).
    tools/time_batch.py --model nnauv|nnspeed [--hid 16|32] [--layers 1..3] [--shape B,K,H] [--only ...] [--steps N] [--reps R]
--model mlp|mlp32|mlp16 [--layers 1..3]: the same four figures for the learned point mass (BatchHandle.learned(model="mlp")):
mlp the [3a, 256, 256, 2a] network (k_rollout_mlp2_batch against lone handles on k_rollout_mlp2), mlp32 / mlp16 Dense(32) / Dense(16) x
--layers (k_rollout_mlp_small_batch against lone DEFAULT handles: k_rollout_mlp32_pc / k_rollout_mlp_small), at a = 3."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mppi_tf_amd as m  # noqa: E402

GOAL = [1, 0, .5, 0, .75, 0, .25, 0]


def kw(K, H, a):
    return dict(k=K, tau=H, s_dim=2 * a, a_dim=a, dt=0.1, lam=1.0, sigma=0.25 * np.eye(a), goal=GOAL[:2 * a])


def auv_kw(K, H):
    """the reference's AUV task as Handle / BatchHandle keywords (seed and x0 dropped: the caller gives the seeds, x0 is the state)"""
    from mppi_tf_amd.auv import auv_task
    t = auv_task(H)
    return {k: v for k, v in t.items() if k not in ("seed", "x0")} | dict(k=K), np.asarray(t["x0"], np.float32)


def configs(model, K, H, a):
    """-> (keywords of Handle / BatchHandle, x0 of one controller)"""
    if model == "auv":
        return auv_kw(K, H)
    return kw(K, H, a), np.zeros(2 * a, np.float32)


def clock(enqueue, sync, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        enqueue()
    sync()
    return time.perf_counter() - t0


def shape(B, K, H, a, steps, reps, only=None, model="pm"):
    a_kw, x0 = configs(model, K, H, a)
    a, s = a_kw["a_dim"], a_kw["s_dim"]
    hb = m.BatchHandle(n=B, **a_kw)
    xb, ub = torch.from_numpy(np.tile(x0, (B, 1))).cuda(), torch.zeros((B, a), device="cuda")
    hs = [m.Handle(seed=1 + i, **a_kw) for i in range(B)]
    xs, us = [torch.from_numpy(x0.copy()).cuda() for _ in hs], [torch.zeros(a, device="cuda") for _ in hs]
    assert xb.shape == (B, s)
    h1 = hs[0]

    def sync_all():
        torch.cuda.synchronize()
        hb.synchronize()
        for h in hs:
            h.synchronize()

    runs = {
        "batch": (lambda: hb.next_device(xb.data_ptr(), ub.data_ptr(), None), hb.synchronize),
        "streams": (lambda: [h.next_device(x.data_ptr(), u.data_ptr(), None) for h, x, u in zip(hs, xs, us)], sync_all),
        "single": (lambda: h1.next_device(xs[0].data_ptr(), us[0].data_ptr(), None), h1.synchronize),
    }
    if only:  # (a kernel-trace run of one of the three: the others' kernels stay out of its statistics)
        runs = {only: runs[only]}
    for f, s in runs.values():  # warm-up: code objects loaded, LDS ceilings raised, clocks up
        clock(f, s, max(50, steps // 4))
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, (f, s) in runs.items():
            t[k].append(clock(f, s, steps) / steps)
    med = {k: float(np.median(v)) for k, v in t.items()}
    per = {"batch": B, "streams": B, "single": 1}
    for k in med:
        w = med[k]
        print("B=%-2d K=%-5d H=%-3d a=%d  %-7s %8.2f us per %s  %7.2f us per controller step  %.3g rollouts/s" % (
            B, K, H, a, k, w * 1e6, "batched step" if k == "batch" else ("round of %d" % B if k == "streams" else "step"),
            w * 1e6 / per[k], per[k] * K / w), flush=True)
    if not only:
        print("B=%-2d K=%-5d H=%-3d a=%d  batch / streams = %.3f   (spread over %d reps: batch %.2f-%.2f us, streams %.2f-%.2f us)" % (
            B, K, H, a, med["batch"] / med["streams"], reps, min(t["batch"]) * 1e6, max(t["batch"]) * 1e6,
            min(t["streams"]) * 1e6, max(t["streams"]) * 1e6), flush=True)
    hb.close()
    for h in hs:
        h.close()
    return med


def learned_net(model, hid, layers, seed, a=3):
    """a random network of the learned model's shape with a normalisation (what the tests use)"""
    rng = np.random.default_rng(seed)
    ends = (3 * a, 2 * a) if model == "mlp" else (16, 13) if model == "nnauv" else (15, 6)
    dims = [ends[0]] + [hid] * layers + [ends[1]]
    W = [(rng.uniform(-1, 1, (dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(layers + 1)]
    b = [(rng.uniform(-1, 1, dims[i + 1]) / np.sqrt(dims[i])).astype(np.float32) for i in range(layers + 1)]
    W[-1] *= 0.1
    b[-1] *= 0.1
    return dict(W=W, b=b, xmean=rng.uniform(-0.1, 0.1, dims[0]).astype(np.float32), xstd=rng.uniform(0.8, 1.2, dims[0]).astype(np.float32),
                ymean=rng.uniform(-0.01, 0.01, dims[-1]).astype(np.float32), ystd=rng.uniform(0.8, 1.2, dims[-1]).astype(np.float32))


def learned(B, K, H, model, hid, layers, steps, reps, only=None, a=3):
    """one network per member: the batch (distinct networks / one shared network) against B lone default handles, serially and on B streams"""
    if model.startswith("mlp"):  # the learned point mass
        kind, s, net_kw, ctl_kw = "mlp", 2 * a, "mlp", dict(a_dim=a)
        c = dict(k=K, tau=H, dt=0.1, lam=1.0, sigma=0.25 * np.eye(a), goal=GOAL[:s], Q=np.array([10.0, 1.0] * a))
        x0 = np.array([0.1, 0, -0.2, 0, 0.3, 0, 0.05, 0][:s], np.float32)
    else:
        kind, s, a, ctl_kw = "nnauv" if model == "nnauv" else "nnauv_speed", 13, 6, {}
        net_kw = kind
        c = dict(k=K, tau=H, dt=0.1, lam=1.0, sigma=0.25 * np.eye(6), goal=[1.0, 2.0, -3.0, 0, 0, np.sin(0.2), np.cos(0.2)] + [0.0] * 6,
                 Q=np.array([10.0] * 3 + [5.0] * 4 + [1.0] * 6))
        x0 = np.array([0.5, -0.5, 0.2, 0.0, 0.0, 0.0, 1.0, 0.3, 0.0, -0.1, 0.0, 0.05, 0.0], np.float32)
    nets = [learned_net(kind if kind == "mlp" else model, hid, layers, 100 + i, a) for i in range(B)]
    seeds = [1 + i for i in range(B)]
    want = (lambda k: only in (None, k))
    hb = m.BatchHandle.learned(B, nets, kind, seeds=seeds, **ctl_kw, **c) if want("batch") else None
    hsh = m.BatchHandle.learned(B, nets[0], kind, seeds=seeds, **ctl_kw, **c) if want("shared") else None
    hs = [m.Handle(seed=seeds[i], s_dim=s, a_dim=a, **{net_kw: nets[i]}, **c) for i in range(B)] if (want("serial") or want("streams")) else []
    xb, ub = torch.from_numpy(np.tile(x0, (B, 1))).cuda(), torch.zeros((B, a), device="cuda")
    xs, us = [torch.from_numpy(x0.copy()).cuda() for _ in hs], [torch.zeros(a, device="cuda") for _ in hs]
    one = torch.cuda.Stream()
    torch.cuda.synchronize()
    names = dict(batch=hb.rollout_kernel_name() if hb else None, lone=hs[0].rollout_kernel_name() if hs else None)

    def sync_all():
        torch.cuda.synchronize()
        for h in hs:
            h.synchronize()

    runs = {}
    if hb:
        runs["batch"] = (lambda: hb.next_device(xb.data_ptr(), ub.data_ptr(), None), hb.synchronize)
    if hsh:
        runs["shared"] = (lambda: hsh.next_device(xb.data_ptr(), ub.data_ptr(), None), hsh.synchronize)
    if hs and want("serial"):
        runs["serial"] = (lambda: [h.next_device(x.data_ptr(), u.data_ptr(), one) for h, x, u in zip(hs, xs, us)], one.synchronize)
    if hs and want("streams"):
        runs["streams"] = (lambda: [h.next_device(x.data_ptr(), u.data_ptr(), None) for h, x, u in zip(hs, xs, us)], sync_all)
    for f, sy in runs.values():
        clock(f, sy, max(20, steps // 4))
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, (f, sy) in runs.items():
            t[k].append(clock(f, sy, steps) / steps)
    med = {k: float(np.median(v)) for k, v in t.items()}
    tag = "%s %dx%d B=%-3d K=%-5d H=%-3d" % (model, hid, layers, B, K, H)
    what = dict(batch="batched step, B networks", shared="batched step, ONE network", serial="round of %d on one stream" % B,
                streams="round of %d on %d streams" % (B, B))
    for k in med:
        print("%s  %-7s %9.2f us per %-28s (min %.2f, max %.2f over %d reps)  %8.2f us per controller step" % (
            tag, k, med[k] * 1e6, what[k], min(t[k]) * 1e6, max(t[k]) * 1e6, reps, med[k] * 1e6 / B), flush=True)
    if "batch" in med and "serial" in med:
        print("%s  serial / batch = %.2f ; the slowest batch rep against the fastest serial rep: %.2f ; kernels %s | %s" % (
            tag, med["serial"] / med["batch"], min(t["serial"]) / max(t["batch"]), names["batch"], names["lone"]), flush=True)
    for k, h in (("batch", hb), ("shared", hsh)):  # the rollout kernel alone, from its dispatch's own begin / end
        if h:
            n = min(steps, 200)
            h.profile_begin(n)
            clock(runs[k][0], runs[k][1], n)
            r, f, got = h.profile_end()
            print("%s  %-7s rollout kernel %.2f us, finish %.2f us (mean of %d dispatches)" % (tag, k, r * 1e3, f * 1e3, got), flush=True)
    for h in [hb, hsh] + hs:
        if h:
            h.close()
    return med


def sweep_kw(B, a_kw):
    """the per-member keywords of the sweep batch: lambda log-spaced over two decades, Sigma and Q scaled by 0.5 .. 2"""
    sc = np.linspace(0.5, 2.0, B)
    sig, Q = np.asarray(a_kw["sigma"], np.float32), np.asarray(a_kw.get("Q", np.ones(a_kw["s_dim"])), np.float32)
    return dict(lams=list(np.logspace(-1, 1, B)), sigmas=np.stack([f * sig for f in sc]), Qs=np.stack([f * Q for f in sc[::-1]]))


def sweep(B, K, H, a, model, steps, reps, only=None):
    a_kw, x0 = configs(model, K, H, a)
    a, s = a_kw["a_dim"], a_kw["s_dim"]
    hs = {}
    if only != "sweep":
        hs["uniform"] = m.BatchHandle(n=B, **a_kw)
    if only != "uniform":
        hs["sweep"] = m.BatchHandle(n=B, **a_kw, **sweep_kw(B, a_kw))
    xb, ub = torch.from_numpy(np.tile(x0, (B, 1))).cuda(), torch.zeros((B, a), device="cuda")
    assert xb.shape == (B, s)
    runs = {k: ((lambda h=h: h.next_device(xb.data_ptr(), ub.data_ptr(), None)), h.synchronize) for k, h in hs.items()}
    for f, sy in runs.values():
        clock(f, sy, max(50, steps // 4))
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, (f, sy) in runs.items():
            t[k].append(clock(f, sy, steps) / steps)
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k in med:
        print("B=%-2d K=%-5d H=%-3d a=%d  %-7s %8.2f us per batched step  (spread over %d reps: %.2f-%.2f us)" % (
            B, K, H, a, k, med[k] * 1e6, reps, min(t[k]) * 1e6, max(t[k]) * 1e6), flush=True)
    if len(med) == 2:
        print("B=%-2d K=%-5d H=%-3d a=%d  sweep / uniform = %.3f" % (B, K, H, a, med["sweep"] / med["uniform"]), flush=True)
    for h in hs.values():
        h.close()
    return med


def main_sweep(o):
    shapes = [("pm", 16, 4096, 64, 2), ("pm", 16, 3000, 50, 3), ("auv", 16, 4096, 40, 6)]
    if o.dry_run:
        for model, B, K, H, a in shapes:
            c, _ = configs(model, K, H, a)
            kw_ = sweep_kw(B, c)
            print("%s B=%-2d K=%-5d H=%-3d a=%d  lambda %.3g..%.3g  %s" % (model, B, K, H, c["a_dim"], kw_["lams"][0], kw_["lams"][-1],
                                                                       sorted(c) + sorted(kw_)), flush=True)
        return
    from mppi_tf_amd import _lib
    print("tools/time_batch.py --sweep: %s, %s, steps %d, reps %d" % (torch.cuda.get_device_name(0), _lib.SO_PATH, o.steps, o.reps), flush=True)
    for model, B, K, H, a in shapes:
        sweep(B, K, H, a, model, o.steps, o.reps, o.only)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="one shape only: B = 4, K = 4096, H = 64, a = 2")
    ap.add_argument("--only", choices=("batch", "streams", "single", "sweep", "uniform", "shared", "serial"),
                    help="time one of the three alone (--sweep: the sweep or the uniform batch alone)")
    ap.add_argument("--sweep", action="store_true", help="a per-member parameter sweep against the uniform batch of the same shape")
    ap.add_argument("--model", choices=("pm", "auv", "nnauv", "nnspeed", "mlp", "mlp32", "mlp16"), default="pm",
                    help="pm: the point mass; auv: the Fossen AUV at the reference's task; nnauv / nnspeed: the learned 13-state models, one network "
                         "per member; mlp / mlp32 / mlp16: the learned point mass (2 x 256, Dense(32), Dense(16)), one network per member")
    ap.add_argument("--hid", type=int, choices=(16, 32), default=32, help="nnauv / nnspeed: the hidden width")
    ap.add_argument("--layers", type=int, choices=(1, 2, 3), default=3, help="nnauv / nnspeed: hidden layers")
    ap.add_argument("--shape", help="one shape only: B,K,H (the action dimension: 2 for pm, 6 for auv)")
    ap.add_argument("--dry-run", action="store_true", help="print the shapes and build their configurations, time nothing (no GPU)")
    o = ap.parse_args()
    if o.sweep:
        return main_sweep(o)
    if o.model in ("nnauv", "nnspeed", "mlp", "mlp32", "mlp16"):
        if o.model.startswith("mlp"):
            o.hid, o.layers = {"mlp": (256, 2), "mlp32": (32, o.layers), "mlp16": (16, o.layers)}[o.model]
        shapes = [(B, 1024, 32) for B in (8, 32, 128)]
        if o.shape:
            shapes = [tuple(int(v) for v in o.shape.split(","))]
        if o.dry_run:
            for B, K, H in shapes:
                print("%s %dx%d B=%-3d K=%-5d H=%-3d" % (o.model, o.hid, o.layers, B, K, H), flush=True)
            return
        print("tools/time_batch.py: %s, model %s %dx%d, steps %d, reps %d" % (torch.cuda.get_device_name(0), o.model, o.hid, o.layers, o.steps,
                                                                           o.reps), flush=True)
        for B, K, H in shapes:
            learned(B, K, H, o.model, o.hid, o.layers, o.steps, o.reps, o.only)
        return
    if o.model == "auv":
        shapes = ([(B, 4096, 40, 6) for B in (1, 2, 4, 8, 16)] + [(B, 16384, 40, 6) for B in (1, 2, 4, 8, 16)]
                  + [(B, 65536, 64, 6) for B in (1, 2)])
        quick = (16, 4096, 40, 6)
    else:
        shapes = ([(B, 4096, 64, 2) for B in (1, 2, 4, 8, 16)] + [(B, 3000, 50, 2) for B in (1, 2, 4, 8, 16)]
                  + [(B, 65536, 64, 3) for B in (1, 2, 4)])
        quick = (4, 4096, 64, 2)
    if o.quick:
        shapes = [quick]
    if o.shape:
        B, K, H = (int(v) for v in o.shape.split(","))
        shapes = [(B, K, H, 6 if o.model == "auv" else 2)]
    if o.dry_run:
        for B, K, H, a in shapes:
            c, x0 = configs(o.model, K, H, a)
            print("B=%-2d K=%-5d H=%-3d a=%d  %s" % (B, K, H, c["a_dim"], sorted(c)), flush=True)
        return
    print("tools/time_batch.py: %s, %s, model %s, steps %d, reps %d" % (torch.cuda.get_device_name(0), m.__name__, o.model, o.steps, o.reps),
          flush=True)
    for B, K, H, a in shapes:
        shape(B, K, H, a, o.steps, o.reps, o.only, o.model)


if __name__ == "__main__":
    main()
