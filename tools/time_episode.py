"""A closed loop on the device against the host loop it replaces, at one grid, in one process. Per control step of the whole batch:
  (a) host:    the loop of examples/sweep.py without --on-device: hb.next(X) (host-synchronous), u to the host, the numpy plant, x back;
  (b) episode: BatchHandle.run_episode: `steps` steps enqueued on the handle's stream, the point-mass model as the plant on the device,
               one synchronisation and one copy of the trajectory at the end;
  (c) floor:   `steps` back-to-back mppi_batch_next_device calls on one x, no plant, one synchronisation: what the controller alone costs.
With --plant the episode of (b) steps the state with SEPARATE plant handles (run_episode(..., plant=)), twins of the controller's model so
that the work is the same: `shared` one plant handle for every member, `members` a plant handle per member (a table of B distinct pointers).
Each figure is a host clock around `steps` steps; the three alternate, `reps` times, and the median is printed in us per batched step.
Grids: the default grid of examples/sweep.py (5 x 4 x 5 x 3 = 300 members, its config and task files) and B = 1 (its first point).
With --stats, instead: what logging the step statistics costs (run_episode(..., stats=True): one k_step_stats launch per step, ONE workgroup
per member) — the episode with and without them, alternating, median per step — at BASELINE configs[1] (point mass a = 2, K = 4096, H = 64:
the one-launch step), configs[2] (a = 3, K = 65536, H = 64: one workgroup reads 256 KB of costs twice) and a batch of 32 point-mass
controllers (the sweep's first 32 grid points). profiles/episode_stats_time.txt keeps the output.
    tools/time_episode.py [--steps N] [--reps R] [--samples K] [--only host|episode|floor] [--plant shared|members] [--stats] [--dry-run]"""
import argparse
import itertools
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import yaml  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
GRID = dict(lams=[0.05, 0.07, 0.1, 0.15, 0.2], upsilons=[1.0, 1.4, 1.8, 2.0], gammas=[0.05, 0.07, 0.1, 0.15, 0.2], noises=[0.10, 0.15, 0.20])


def sweep_kw(samples, B):
    """BatchHandle's keywords of the first B points of the sweep's default grid (examples/sweep.py main) -> (keywords, dt, mass)"""
    with open(os.path.join(ROOT, "examples", "config", "point_mass3d.yaml")) as fh:
        conf = yaml.safe_load(fh)
    with open(os.path.join(ROOT, "examples", "config", "static_task3d.yaml")) as fh:
        task = yaml.safe_load(fh)
    s, a, dt, mass = conf["state-dim"], conf["action-dim"], float(conf["dt"]), float(conf["mass"])
    grid = list(itertools.product(GRID["lams"], GRID["upsilons"], GRID["gammas"], GRID["noises"]))[:B]
    n = len(grid)
    return dict(n=n, k=samples or conf["samples"], tau=conf["horizon"], s_dim=s, a_dim=a, dt=dt, mass=mass, goal=np.asarray(task["goal"], np.float32),
                Q=np.asarray(task["Q"], np.float32), action_cost=1, upsilon_scales_noise=True, seeds=[1] * n, lams=[g[0] for g in grid],
                upsilons=[g[1] for g in grid], gammas=[g[2] for g in grid], sigmas=[g[3] * np.eye(a, dtype=np.float32) for g in grid]), dt, mass


def time_grid(m, B, samples, steps, reps, only=None, plants=None):
    import torch
    from sweep import plant
    kw, dt, mass = sweep_kw(samples, B)
    n, s, a = kw["n"], kw["s_dim"], kw["a_dim"]
    # the plant handles of --plant: the controller's own point mass again (k = 1, tau = 1: they run no rollouts)
    ps = [m.Handle(k=1, tau=1, s_dim=s, a_dim=a, dt=dt, mass=mass) for _ in range({None: 0, "shared": 1, "members": n}[plants])]
    ep_plant = None if plants is None else (ps[0] if plants == "shared" else ps)
    ep_name = "episode" if plants is None else "episode (plant: %s)" % plants
    hs = {k: m.BatchHandle(**kw) for k in ("host", "episode", "floor") if only in (None, k)}  # a handle each: the three never share a sequence
    xd, ud = torch.zeros((n, s), device="cuda"), torch.zeros((n, a), device="cuda")
    torch.cuda.synchronize()

    def host(h, k):
        X = np.zeros((n, s), np.float32)
        for _ in range(k):
            X = plant(X, h.next(X), dt, mass)

    def episode(h, k):
        h.run_episode(np.zeros((n, s), np.float32), k, plant=ep_plant)

    def floor(h, k):
        for _ in range(k):
            h.next_device(xd.data_ptr(), ud.data_ptr(), None)
        h.synchronize()
    runs = {k: (f, hs[k]) for k, f in (("host", host), ("episode", episode), ("floor", floor)) if k in hs}
    for f, h in runs.values():  # warm-up: code objects loaded, LDS ceilings raised, the staging allocated, clocks up
        f(h, max(10, steps // 4))
        f(h, steps)
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, (f, h) in runs.items():
            t0 = time.perf_counter()
            f(h, steps)
            t[k].append((time.perf_counter() - t0) / steps)
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k, w in med.items():
        print("B=%-3d K=%-5d H=%-3d a=%d  %-7s %9.2f us per batched step  (spread over %d reps: %.2f-%.2f us)" % (
            n, kw["k"], kw["tau"], a, ep_name if k == "episode" else k, w * 1e6, reps, min(t[k]) * 1e6, max(t[k]) * 1e6), flush=True)
    if len(med) == 3:
        print("B=%-3d K=%-5d H=%-3d a=%d  episode / host = %.3f   episode - floor = %.2f us per step" % (
            n, kw["k"], kw["tau"], a, med["episode"] / med["host"], (med["episode"] - med["floor"]) * 1e6), flush=True)
    for h in list(hs.values()) + ps:
        h.close()
    return med


def stats_cases(samples):
    """name -> (class name, keywords, x0 shape) of the three --stats cases"""
    pm = lambda a, K: dict(k=K, tau=64, s_dim=2 * a, a_dim=a, dt=0.1, mass=1.0, lam=1.0, sigma=(0.25 * np.eye(a)).astype(np.float32),
                           goal=[1.0, 0.0, 0.5, 0.0, 0.75, 0.0][:2 * a], seed=1)
    kw32 = sweep_kw(samples, 32)[0]
    return {"configs[1] K=4096 H=64 a=2": ("Handle", pm(2, 4096), (4,)), "configs[2] K=65536 H=64 a=3": ("Handle", pm(3, 65536), (6,)),
            "batch B=32 K=%d H=%d a=%d" % (kw32["k"], kw32["tau"], kw32["a_dim"]): ("BatchHandle", kw32, (32, kw32["s_dim"]))}


def time_stats(m, samples, steps, reps):
    for name, (cls, kw, shape) in stats_cases(samples).items():
        hs = {False: getattr(m, cls)(**kw), True: getattr(m, cls)(**kw)}  # a handle each: the two never share a sequence
        x0 = np.zeros(shape, np.float32)
        for stats, h in hs.items():  # warm-up: code objects loaded, the staging allocated, clocks up
            h.run_episode(x0, max(10, steps // 4), stats=stats)
            h.run_episode(x0, steps, stats=stats)
        t = {False: [], True: []}
        for _ in range(reps):
            for stats, h in hs.items():
                t0 = time.perf_counter()
                h.run_episode(x0, steps, stats=stats)
                t[stats].append((time.perf_counter() - t0) / steps)
        plain, logged = (float(np.median(t[k])) * 1e6 for k in (False, True))
        print("%-30s episode %8.2f us per step, with statistics %8.2f us (%.2f-%.2f over %d reps): +%.2f us per step = %.0f %% of the step"
              % (name, plain, logged, min(t[True]) * 1e6, max(t[True]) * 1e6, reps, logged - plain, 100.0 * (logged - plain) / plain), flush=True)
        for h in hs.values():
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="steps per timed loop (the sweep's default: 300)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=None, help="samples per member (default: the sweep config's)")
    ap.add_argument("--only", choices=("host", "episode", "floor"), help="time one of the three alone")
    ap.add_argument("--plant", choices=("shared", "members"), help="the episode steps the state with separate plant handles, twins of the "
                                                                   "controller's model: one for all members, or one per member")
    ap.add_argument("--stats", action="store_true", help="time the episode with and without the step statistics instead (three cases)")
    ap.add_argument("--dry-run", action="store_true", help="print the grids and build their keywords, time nothing (no GPU)")
    o = ap.parse_args()
    grids = (300, 1)
    if o.dry_run:
        for name, (cls, kw, shape) in (stats_cases(o.samples).items() if o.stats else ()):
            print("--stats %-30s %s x0 %s %s" % (name, cls, shape, sorted(kw)), flush=True)
        for B in grids:
            kw, dt, mass = sweep_kw(o.samples, B)
            print("B=%-3d K=%-5d H=%-3d a=%d  dt %g mass %g  %s" % (kw["n"], kw["k"], kw["tau"], kw["a_dim"], dt, mass, sorted(kw)), flush=True)
        return
    import torch
    import mppi_tf_amd as m
    print("tools/time_episode.py: %s, steps %d, reps %d" % (torch.cuda.get_device_name(0), o.steps, o.reps), flush=True)
    if o.stats:
        return time_stats(m, o.samples, o.steps, o.reps)
    for B in grids:
        time_grid(m, B, o.samples, o.steps, o.reps, o.only, o.plant)


if __name__ == "__main__":
    main()
