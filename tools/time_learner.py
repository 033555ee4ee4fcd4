"""The wide learner's Adam step against the clock, against torch on the same GPU, and against the narrow learner, in one process.
For the [9, 256, 256, 6] network at n in {1024, 8192, 65536} samples:
  (a) wide:   Learner.train(200) — 200 full-batch Adam steps enqueued by one call that synchronises once (csrc/mppi_learner_wide.hip);
  (b) torch:  the same network, loss and optimiser in torch on the same GPU: fp32, torch.backends.cuda.matmul.allow_tf32 = False,
              torch.optim.Adam(eps=1e-7), 200 steps in one Python loop, synchronised once;
  (c) narrow: Learner.train(200) of the [16, 32, 32, 32, 13] network at the same n, for scale.
Each figure is a host clock around work that ends in one device synchronisation, after a warm-up call of the same shape; (a), (b), (c)
alternate `reps` times and the median is printed in microseconds per step with the spread. The FLOP count of a wide step is the three
GEMM passes (forward, delta, weight gradient) over the three layers, 3 x 2 n (in 256 + 256 256 + 256 out); the peak it is set against is
the 157.3 TFLOP/s of the exact-fp32 matrix-core instruction. This is a whole-step rate (nine launches, their gaps included), not a
kernel's share of peak.
    tools/time_learner.py [--reps R] [--steps S] [--out FILE] [--dry-run]
With --batch B[,B...] it times batched learners instead: for the [16, 32, 32, 32, 13] network at n in --ns (264, 4096) rows, B learners that
each train on all n rows, as
  (d) batch:      one LearnerBatch of B members, train(steps) (csrc/mppi_learner_batch.hip: 3 launches per step for all members);
  (e) sequential: B lone Learners, train(steps) one after another (3 B launches per step of the set);
  (f) threads:    the same B lone Learners, train(steps) from B host threads at once, each learner on its own stream.
The same clock, warm-up, alternation and medians; the figure is microseconds per Adam step OF THE WHOLE SET (all B learners advance one
step). No held-out rows: the lone learners have no test pass to set against one. After the timing every batch member's weights are
compared with a lone learner's (they made the same number of steps from the same start): the bits must be equal.
    tools/time_learner.py --batch 10,100 [--ns 264,4096] [--reps R] [--steps S] [--out FILE]
With --batch B[,B...] --wide the same table is taken for the [9, 256, 256, 6] network: (d) is one WideLearnerBatch of B members
(csrc/mppi_learner_wide_batch.hip: 9 launches per step for all members), (e) and (f) are B lone wide Learners (9 B launches per step of the set).
    tools/time_learner.py --batch 10,100 --wide [--ns 264,4096] [--reps R] [--steps S] [--out profiles/learner_wide_batch_time.txt]
With --batch B[,B...] --validate it times the trajectory validation of a batch instead (csrc/mppi_learner_rollout.hip): the NNAUVModel network
[16, 32, 32, 32, 13], B members of different weights, n trajectories (--ns, default 16 and 256) of T = 50 steps, as
  (g) batch: one LearnerBatch.rollout(model, x0, V, gt=G) — every member in ONE launch, the squared errors summed on the device;
  (h) lone:  B lone handles that already hold the members' weights, each Handle.model_rollout(x0, V, costs=False) (T + 1 launches) and the
             squared error of the returned trajectory summed on the host — the only way to these numbers without the batch's kernel.
             Creating the B handles and pushing the members' weights into them is timed once, apart.
The same clock, warm-up, alternation and medians; the figure is microseconds per validation of the whole set. Afterwards every member's
trajectory is compared with its handle's: the bits must be equal.
    tools/time_learner.py --batch 10,100 --validate [--ns 16,256] [--reps R] [--out FILE]
With --batch B[,B...] --wide --validate the same comparison is taken for the wide members (csrc/mppi_learner_wide_rollout.hip): the
[9, 256, 256, 6] point-mass network, n = 16 trajectories (--ns) of T = 50 steps; (g) is one WideLearnerBatch.validate, (h) B lone
MPPI_MODEL_MLP handles' model_rollout one after another (T launches each of a kernel that runs one thread per trajectory). One pass over
the lone handles takes seconds, so a sample of `lone` is ONE pass where a sample of `batch` is ten calls.
    tools/time_learner.py --batch 10,100 --wide --validate [--ns 16] [--reps R] [--out profiles/learner_wide_batch_validate_time.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

F32 = np.float32
WIDE, NARROW = [9, 256, 256, 6], [16, 32, 32, 32, 13]
NS = (1024, 8192, 65536)
PEAK_TFLOPS = 157.3


def make_net(dims, seed=0):
    rng = np.random.default_rng(seed)
    return dict(W=[(rng.uniform(-1, 1, (dims[i], dims[i + 1])) * np.sqrt(6.0 / (dims[i] + dims[i + 1]))).astype(F32) for i in range(len(dims) - 1)],
                b=[np.zeros(dims[i + 1], F32) for i in range(len(dims) - 1)])


def make_data(dims, n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, dims[0])).astype(F32)
    return X, np.tanh(X @ rng.standard_normal((dims[0], dims[-1])) * 0.3).astype(F32)


def step_flops(dims, n):
    return 3 * 2 * n * sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))


def torch_trainer(net, X, Y, lr):
    import torch
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    Ws = [torch.tensor(w, device="cuda", requires_grad=True) for w in net["W"]]
    bs = [torch.tensor(b, device="cuda", requires_grad=True) for b in net["b"]]
    dX, dY = torch.tensor(X, device="cuda"), torch.tensor(Y, device="cuda")
    opt = torch.optim.Adam(Ws + bs, lr=lr, eps=1e-7)

    def train(steps):
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            h = dX
            for l in range(len(Ws)):
                h = torch.addmm(bs[l], h, Ws[l])
                if l + 1 < len(Ws):
                    h = torch.relu(h)
            loss = torch.mean((h - dY) ** 2)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return float(loss.detach())
    return train


def time_batch(o):
    import threading
    import torch
    import mppi_tf_amd as m
    lr = 1e-3
    dims, Batch, name = (WIDE, m.WideLearnerBatch, "WideLearnerBatch") if o.wide else (NARROW, m.LearnerBatch, "LearnerBatch")
    head = ["tools/time_learner.py --batch%s: %s, [%s], %d Adam steps per call, reps %d; medians of a host clock around calls that end in one" % (
        " --wide" if o.wide else "", torch.cuda.get_device_name(0), ",".join(str(d) for d in dims), o.steps, o.reps),
        "synchronisation each (every learner enqueues on its own stream); microseconds per Adam step of the whole set of B learners (min-max), alternating rounds;",
        "batch = one %s of B members, sequential = B lone Learners one after another, threads = the same B Learners from B host threads at once" % name]
    print("\n".join(head), flush=True)
    lines = list(head)
    net = make_net(dims)
    for n in o.ns:
        X, Y = make_data(dims, n)
        for B in o.batch:
            batch = Batch(net, B)
            batch.set_data(X, Y)
            lone = [m.Learner(net) for _ in range(B)]
            for l in lone:
                l.set_data(X, Y)

            def sequential():
                for l in lone:
                    l.train(o.steps, lr)

            def threads():
                ts = [threading.Thread(target=l.train, args=(o.steps, lr)) for l in lone]
                for th in ts:
                    th.start()
                for th in ts:
                    th.join()

            runs = (("batch", lambda: batch.train(o.steps, lr)), ("sequential", sequential), ("threads", threads))
            for _, f in runs:  # warm-up of every shape
                f()
            t = {k: [] for k, _ in runs}
            for _ in range(o.reps):
                for k, f in runs:
                    t0 = time.perf_counter()
                    f()
                    t[k].append((time.perf_counter() - t0) / o.steps * 1e6)
            med = {k: float(np.median(v)) for k, v in t.items()}
            # the lone learners made two calls per round (sequential, threads), the batch one: bring the batch level, then compare bits
            batch.train(o.steps * (o.reps + 1), lr)
            wl = lone[0].get_weights()
            same = all(np.array_equal(a, b) for mi in (0, B - 1) for key in ("W", "b") for a, b in zip(batch.get_weights(mi)[key], wl[key]))
            line = ("n=%-5d B=%-4d batch %9.1f us (%.1f-%.1f)   sequential %9.1f us (%.1f-%.1f)  = %5.2fx batch   threads %9.1f us (%.1f-%.1f)  = %5.2fx batch"
                    "   per learner and step: batch %.2f us, lone %.2f us   members bit-equal to a lone learner after %d steps: %s" % (
                        n, B, med["batch"], min(t["batch"]), max(t["batch"]), med["sequential"], min(t["sequential"]), max(t["sequential"]),
                        med["sequential"] / med["batch"], med["threads"], min(t["threads"]), max(t["threads"]), med["threads"] / med["batch"],
                        med["batch"] / B, med["sequential"] / B, lone[0].step_count(), same and batch.step_count() == lone[0].step_count()))
            print(line, flush=True)
            lines.append(line)
            batch.close()
            for l in lone:
                l.close()
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def time_validate(o):
    import torch
    import mppi_tf_amd as m
    T, CALLS = 50, 10  # a sample of the clock is CALLS validations, each ending in its own synchronisation
    LONE_CALLS = 1 if o.wide else CALLS  # one pass over B lone wide handles takes seconds
    dims, s_dim, a_dim = (WIDE, 6, 3) if o.wide else (NARROW, 13, 6)
    what = "NNPointMassModel [9,256,256,6]" if o.wide else "NNAUVModel [16,32,32,32,13]"
    call = "WideLearnerBatch.validate" if o.wide else "LearnerBatch.rollout"
    head = ["tools/time_learner.py --batch%s --validate: %s, %s, T = %d steps, reps %d of %d calls%s; medians of a host clock around calls that end" % (
        " --wide" if o.wide else "", torch.cuda.get_device_name(0), what, T, o.reps, CALLS, " (lone: of %d)" % LONE_CALLS if LONE_CALLS != CALLS else ""),
        "in a synchronisation; microseconds per validation of the whole set of B networks (min-max), alternating rounds; batch = one %s" % call,
        "(1 launch, sse on the device), lone = B handles holding the members' weights, each model_rollout (%s launches) + the sse on the host;" % ("T" if o.wide else "T + 1"),
        "setup = creating those B handles with the members' weights, once, not part of `lone`"]
    print("\n".join(head), flush=True)
    lines = list(head)
    norm = dict(xmean=np.zeros(dims[0], F32), xstd=np.ones(dims[0], F32), ymean=np.zeros(dims[-1], F32), ystd=np.ones(dims[-1], F32))
    desc = dict(kind="mlp" if o.wide else "nnauv", s_dim=s_dim, a_dim=a_dim, dt=0.1, **norm)
    for n in o.ns:
        rng = np.random.default_rng(n)
        x0 = np.zeros((n, s_dim), F32)
        if o.wide:
            x0[:] = rng.uniform(-1, 1, (n, s_dim))
        else:
            x0[:, :3], x0[:, 6], x0[:, 7:] = rng.uniform(-1, 1, (n, 3)), 1.0, rng.uniform(-0.3, 0.3, (n, 6))
        V = rng.standard_normal((T, n, a_dim)).astype(F32)
        G = (np.broadcast_to(x0, (T + 1, n, s_dim)) + 0.05 * rng.standard_normal((T + 1, n, s_dim))).astype(F32)
        for B in o.batch:
            nets = [make_net(dims, seed) for seed in range(B)]
            for net in nets:
                net["W"][-1] *= F32(0.1)
            batch = (m.WideLearnerBatch if o.wide else m.LearnerBatch)(nets[0], B)
            for i, net in enumerate(nets):
                batch.set_weights(net, member=i)
            roll = batch.validate if o.wide else batch.rollout
            t0 = time.perf_counter()
            kw = dict(k=1, tau=1, s_dim=s_dim, a_dim=a_dim, dt=0.1, sigma=np.eye(a_dim, dtype=F32), goal=np.zeros(s_dim, F32))
            lone = [m.Handle(**kw, **{"mlp" if o.wide else "nnauv": dict(net, **norm)}) for net in nets]
            setup = (time.perf_counter() - t0) * 1e6
            G64 = G.astype(np.float64)

            def lone_all():
                return np.stack([((h.model_rollout(x0, V, costs=False)[0].astype(np.float64) - G64) ** 2).sum(axis=(0, 1)) for h in lone])

            runs = (("batch", lambda: roll(desc, x0, V, gt=G)["sse"], CALLS), ("lone", lone_all, LONE_CALLS))
            got = {k: f() for k, f, _ in runs}  # warm-up of every shape
            t = {k: [] for k, _, _ in runs}
            for _ in range(o.reps):
                for k, f, calls in runs:
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        f()
                    t[k].append((time.perf_counter() - t0) / calls * 1e6)
            med = {k: float(np.median(v)) for k, v in t.items()}
            X = roll(desc, x0, V, trajectories=True)["X"]
            same = all(np.array_equal(X[i], lone[i].model_rollout(x0, V, costs=False)[0]) for i in range(B))
            rel = float(np.max(np.abs(got["batch"] - got["lone"]) / got["lone"]))
            line = ("n=%-4d B=%-4d batch %9.1f us (%.1f-%.1f)   lone %10.1f us (%.1f-%.1f)  = %6.2fx batch   per network: batch %.1f us, lone %.1f us   setup of the "
                    "lone handles %.0f us   trajectories bit-equal: %s   sse batch vs host fp64: %.2g relative" % (
                        n, B, med["batch"], min(t["batch"]), max(t["batch"]), med["lone"], min(t["lone"]), max(t["lone"]), med["lone"] / med["batch"],
                        med["batch"] / B, med["lone"] / B, setup, same, rel))
            print(line, flush=True)
            lines.append(line)
            batch.close()
            for h in lone:
                h.close()
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=lambda v: [int(x) for x in v.split(",")], help="B[,B...]: time a LearnerBatch of B members against B lone learners")
    ap.add_argument("--ns", type=lambda v: [int(x) for x in v.split(",")], default=None, help="rows of the pool, with --batch (264,4096); trajectories, with --validate (16,256)")
    ap.add_argument("--wide", action="store_true", help="with --batch: the [9, 256, 256, 6] network, a WideLearnerBatch against B lone wide learners")
    ap.add_argument("--validate", action="store_true", help="with --batch: time LearnerBatch.rollout (--wide: WideLearnerBatch.validate) against B lone handles' model_rollout")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", help="also write the table to this file")
    ap.add_argument("--dry-run", action="store_true", help="build the networks and the data, count the operations, time nothing (no GPU)")
    o = ap.parse_args()
    if o.validate and not o.batch:
        ap.error("--validate goes with --batch")
    if o.wide and not o.batch:
        ap.error("--wide goes with --batch")
    o.ns = o.ns or (([16] if o.wide else [16, 256]) if o.validate else [264, 4096])
    if o.batch and not o.dry_run:
        return time_validate(o) if o.validate else time_batch(o)
    if o.dry_run:
        for n in NS:
            X, Y = make_data(WIDE, n)
            print("n=%-6d X %s Y %s  wide step %.4g GFLOP  narrow step %.4g GFLOP" % (n, X.shape, Y.shape, step_flops(WIDE, n) / 1e9, step_flops(NARROW, n) / 1e9))
        return
    import torch
    import mppi_tf_amd as m
    lr = 1e-3
    head = ["tools/time_learner.py: %s, %d Adam steps per call, reps %d; medians of a host clock around one call that ends in one synchronisation," % (
        torch.cuda.get_device_name(0), o.steps, o.reps),
        "microseconds per step (min-max); wide = [9,256,256,6] on the exact-fp32 matrix cores, torch = the same step in torch fp32 (no tf32), narrow = [16,32,32,32,13];",
        "TFLOP/s = 3 x 2 n (9*256 + 256*256 + 256*6) per step over the step time (whole step, launch gaps included), peak %.1f" % PEAK_TFLOPS]
    print("\n".join(head), flush=True)
    lines = list(head)
    for n in NS:
        X, Y = make_data(WIDE, n)
        Xn, Yn = make_data(NARROW, n)
        wide, narrow = m.Learner(make_net(WIDE)), m.Learner(make_net(NARROW))
        wide.set_data(X, Y)
        narrow.set_data(Xn, Yn)
        tt = torch_trainer(make_net(WIDE), X, Y, lr)
        runs = (("wide", lambda: wide.train(o.steps, lr)), ("torch", lambda: tt(o.steps)), ("narrow", lambda: narrow.train(o.steps, lr)))
        first = {k: f() for k, f in runs}  # warm-up of every shape
        t = {k: [] for k, _ in runs}
        for _ in range(o.reps):
            for k, f in runs:
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) / o.steps * 1e6)
        med = {k: float(np.median(v)) for k, v in t.items()}
        tf = step_flops(WIDE, n) / (med["wide"] * 1e-6) / 1e12
        line = ("n=%-6d wide %9.1f us (%.1f-%.1f)  %6.2f TFLOP/s = %4.1f %% of peak   torch %9.1f us (%.1f-%.1f)  torch/wide %5.2fx   narrow %8.1f us (%.1f-%.1f)"
                "   first-call loss wide %.5f -> %.5f, torch last %.5f" % (
                    n, med["wide"], min(t["wide"]), max(t["wide"]), tf, 100.0 * tf / PEAK_TFLOPS, med["torch"], min(t["torch"]), max(t["torch"]),
                    med["torch"] / med["wide"], med["narrow"], min(t["narrow"]), max(t["narrow"]), first["wide"][0], first["wide"][1], first["torch"]))
        print(line, flush=True)
        lines.append(line)
        wide.close()
        narrow.close()
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
