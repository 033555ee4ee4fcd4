"""One open-loop rollout call against the host loop it replaces, per model family, in one process. For n trajectories of T steps:
  (a) loop:    T x (Handle.model_next + Handle.state_cost) on the n rows — one mppi_model_step and one mppi_state_cost call per step, each of
               which allocates scratch, copies in, launches, copies out and synchronises: the only way to do this before mppi_model_rollout;
  (b) rollout: ONE Handle.model_rollout call (host pointers: allocate, upload, enqueue, download, one synchronisation);
  (c) device:  ONE Handle.model_rollout_device call on resident torch tensors and one synchronisation: what the enqueued work alone costs.
Each figure is a host clock around work that ends in a device synchronisation; the three alternate `reps` times after a warm-up of every
shape, and the median is printed in microseconds per call, with the spread. The results of (a) and (b) are compared bit for bit first.
Families: the point mass (a = 3), the Fossen AUV model (rexrov2, rk 2, StaticQuatCost), a learned point mass (Dense(32), a = 2) and
NNAUVModel (Dense(16)); n in {1, 64, 4096}, T in {20, 64}.
    tools/time_model_rollout.py [--reps R] [--out FILE] [--dry-run]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

F32 = np.float32
NS, TS = (1, 64, 4096), (20, 64)
FAMILIES = ("point mass a=3", "Fossen AUV rk=2", "MLP Dense(32) a=2", "NNAUV Dense(16)")


def mlp_weights(n_in, hid, n_out, seed=0):
    rng = np.random.default_rng(seed)
    dims = [n_in, hid, n_out]
    W = [(rng.uniform(-1, 1, (dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(F32) for i in range(2)]
    b = [(rng.uniform(-1, 1, dims[i + 1]) / np.sqrt(dims[i])).astype(F32) for i in range(2)]
    W[-1] *= 0.1
    b[-1] *= 0.1
    return dict(W=W, b=b, xmean=np.zeros(n_in, F32), xstd=np.ones(n_in, F32), ymean=np.zeros(n_out, F32), ystd=np.ones(n_out, F32))


def handle_kw(family):
    """Handle keywords of one family (k = 64, tau = 4: the rollout reads the model and the cost only)"""
    if family == FAMILIES[0]:
        return dict(k=64, tau=4, s_dim=6, a_dim=3, dt=0.1, mass=1.0, goal=np.asarray([1, 0, .5, 0, .75, 0], F32), Q=np.ones(6, F32))
    if family == FAMILIES[2]:
        return dict(k=64, tau=4, s_dim=4, a_dim=2, dt=0.1, goal=np.asarray([1, 0, .5, 0], F32), Q=np.ones(4, F32), mlp=mlp_weights(6, 32, 4))
    goal = np.zeros(13, F32)
    goal[6] = 1.0
    kw = dict(k=64, tau=4, s_dim=13, a_dim=6, dt=0.1, sigma=np.eye(6, dtype=F32), goal=goal, Q=np.ones(10, F32), quat_cost=True)
    if family == FAMILIES[1]:
        from mppi_tf_amd.auv import auv_task
        return dict(kw, auv=dict(auv_task(8)["auv"], rk=2))
    return dict(kw, nnauv=mlp_weights(16, 16, 13))


def inputs(s, a, n, T, scale):
    rng = np.random.default_rng(n + T)
    x0 = rng.uniform(-0.5, 0.5, (n, s)).astype(F32)
    if s == 13:
        x0[:, 3:7] = [0.0, 0.0, 0.0, 1.0]
    return x0, (scale * rng.standard_normal((T, n, a))).astype(F32)


def time_family(m, family, reps, out):
    import torch
    h = m.Handle(**handle_kw(family))
    for n in NS:
        for T in TS:
            x0, V = inputs(h.s, h.a, n, T, 50.0 if family == FAMILIES[1] else 0.5)
            dx, dV = torch.from_numpy(x0).cuda(), torch.from_numpy(V).cuda()
            dX, dC = torch.zeros((T + 1, n, h.s), device="cuda"), torch.zeros((T, n), device="cuda")
            torch.cuda.synchronize()

            def loop():
                x, X, Cs = x0, [x0], []
                for t in range(T):
                    x = h.model_next(x, V[t])
                    X.append(x)
                    Cs.append(h.state_cost(x))
                return np.stack(X), np.stack(Cs)

            def rollout():
                return h.model_rollout(x0, V)

            def device():
                h.model_rollout_device(dx.data_ptr(), n, dV.data_ptr(), n, T, dX.data_ptr(), dC.data_ptr())
                h.synchronize()
            runs = (("loop", loop), ("rollout", rollout), ("device", device))
            (Xl, Cl), (Xr, Cr) = loop(), rollout()  # warm-up of every shape, and the results agree bit for bit
            device()
            same = np.array_equal(Xl, Xr) and np.array_equal(Cl, Cr) and np.array_equal(dX.cpu().numpy(), Xr) and np.array_equal(dC.cpu().numpy(), Cr)
            for _, f in runs:
                f()
            t = {k: [] for k, _ in runs}
            for _ in range(reps):
                for k, f in runs:
                    t0 = time.perf_counter()
                    f()
                    t[k].append(time.perf_counter() - t0)
            med = {k: float(np.median(v)) * 1e6 for k, v in t.items()}
            line = "%-18s n=%-5d T=%-3d loop %10.1f us (%.1f-%.1f)  rollout %9.1f us (%.1f-%.1f)  device %9.1f us (%.1f-%.1f)  loop/rollout %6.1fx  %s" % (
                family, n, T, med["loop"], min(t["loop"]) * 1e6, max(t["loop"]) * 1e6, med["rollout"], min(t["rollout"]) * 1e6,
                max(t["rollout"]) * 1e6, med["device"], min(t["device"]) * 1e6, max(t["device"]) * 1e6, med["loop"] / med["rollout"],
                "bit-identical" if same else "RESULTS DIFFER")
            print(line, flush=True)
            out.append(line)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", help="also write the table to this file")
    ap.add_argument("--dry-run", action="store_true", help="build every family's keywords and inputs, time nothing (no GPU)")
    o = ap.parse_args()
    if o.dry_run:
        for family in FAMILIES:
            kw = handle_kw(family)
            for n in NS:
                for T in TS:
                    x0, V = inputs(kw["s_dim"], kw["a_dim"], n, T, 1.0)
                    print("%-18s n=%-5d T=%-3d x0 %s V %s" % (family, n, T, x0.shape, V.shape), flush=True)
        return
    import torch
    import mppi_tf_amd as m
    head = ["tools/time_model_rollout.py: %s, reps %d; medians of a host clock around one call that ends in a synchronisation (min-max)" % (
        torch.cuda.get_device_name(0), o.reps),
        "loop = T x (model_next + state_cost), the only way before mppi_model_rollout; rollout = one Handle.model_rollout (host pointers);",
        "device = one Handle.model_rollout_device on resident tensors + one synchronisation"]
    print("\n".join(head), flush=True)
    lines = list(head)
    for family in FAMILIES:
        time_family(m, family, o.reps, lines)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
