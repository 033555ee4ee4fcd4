#!/usr/bin/env python3
"""A controller-parameter sweep as ONE batched controller: every point of a lambda x upsilon x gamma x noise grid is a member of one
BatchHandle with its own lambda, upsilon, gamma and Sigma (BatchHandle's lams / upsilons / gammas / sigmas), and all of them step in the
same two launches. This is the grid the reference sweeps with one process per point (5 x 4 x 5 x 3 = 300 runs of 300 steps):
    python examples/sweep.py                                   # that grid, 300 steps, the point-mass static task
    python examples/sweep.py --lams 0.05 0.2 --upsilons 1 2 --gammas 0.1 --noises 0.1 0.2 -s 5
    python examples/sweep.py --on-device                       # the whole closed loop as ONE call (BatchHandle.run_episode)
    python examples/sweep.py --on-device --plant-mass 0.8,1.0,1.25   # ... on vehicles lighter and heavier than the controller's model
The controller uses the Python action-cost form (gamma, upsilon; ACTION_COST_PY) with upsilon scaling the noise (upsilon_scales_noise).
Plant and controller are the point mass of examples/config/point_mass3d.yaml on the static task examples/config/static_task3d.yaml; noise
n means Sigma = n I. Every member draws its noise from the same Philox key (--seed), as every run of the reference's sweep does. Prints the
final distance to the goal of every grid point.
Without --on-device every step is hb.next(X): a host-synchronous call, u to the host, the numpy plant below, x back. With it the grid's
steps run as one run_episode call: the controller's own point-mass model is the plant, on the device, and the trajectory comes back once.
The two modes print the same table in different digits: the numpy plant holds dt^2/2m rounded once from double, the model divides in
fp32 (one ulp apart), and the closed loop at these temperatures amplifies that to the size of the noise within twenty steps.
With --plant-mass m1,m2,... (and --on-device) the grid runs once per plant mass, all of them as ONE batch: member (point, mass) plans with
the config's mass and its state is stepped by a separate plant handle of that mass (run_episode(..., plant=[...]), a plant per member);
the table gains the plant-mass column and says which setting survives a vehicle that is not the modelled one.
With --on-device the table also says whether each lambda WEIGHS the samples sensibly, from the step statistics the episode logs on the device
(run_episode(..., stats=True)): ess/K, the effective sample size as a share of the samples, mean over the episode (near 1: the update is the
plain mean of the noise; near 1/K: one sample holds all the weight), and needle, the share of steps with an effective sample size below 2.
The reference sweeps its ellipse task; a batch refuses the 2D ellipse cost (ElipseCost), so this sweep runs the static task."""
import argparse
import itertools
import os
import sys
import time

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mppi_tf_amd as m  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def plant(X, U, dt, mass):
    """the point mass, every member at once: x[2j] += dt v + dt^2/2 u/m, v += dt u/m (model_base.cpp:59-82, fp32)"""
    X = X.copy()
    a = U.shape[1]
    bp, bq = np.float32(dt * dt / 2 / mass), np.float32(dt / mass)
    for j in range(a):
        X[:, 2 * j] = X[:, 2 * j] + np.float32(dt) * X[:, 2 * j + 1] + bp * U[:, j]
        X[:, 2 * j + 1] = X[:, 2 * j + 1] + bq * U[:, j]
    return X


def main():
    ap = argparse.ArgumentParser(description="lambda x upsilon x gamma x noise sweep as one batched controller")
    ap.add_argument("--config", default=os.path.join(HERE, "config", "point_mass3d.yaml"))
    ap.add_argument("--task", default=os.path.join(HERE, "config", "static_task3d.yaml"))
    ap.add_argument("--lams", type=float, nargs="+", default=[0.05, 0.07, 0.1, 0.15, 0.2])
    ap.add_argument("--upsilons", type=float, nargs="+", default=[1.0, 1.4, 1.8, 2.0])
    ap.add_argument("--gammas", type=float, nargs="+", default=[0.05, 0.07, 0.1, 0.15, 0.2])
    ap.add_argument("--noises", type=float, nargs="+", default=[0.10, 0.15, 0.20])
    ap.add_argument("-s", "--steps", type=int, default=300)
    ap.add_argument("--samples", type=int, default=None, help="samples per member (default: the config's)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--on-device", action="store_true", help="run all steps as one BatchHandle.run_episode call (the model is the plant)")
    ap.add_argument("--plant-mass", type=lambda v: [float(x) for x in v.split(",")], default=None, metavar="m1,m2,...",
                    help="with --on-device: run the grid once per plant mass, as one batch with a plant handle per member")
    o = ap.parse_args()
    if o.plant_mass and not o.on_device:
        ap.error("--plant-mass needs --on-device (the host loop's plant is the config's point mass)")
    with open(o.config) as fh:
        conf = yaml.safe_load(fh)
    with open(o.task) as fh:
        task = yaml.safe_load(fh)
    s, a, dt, mass = conf["state-dim"], conf["action-dim"], float(conf["dt"]), float(conf["mass"])
    goal = np.asarray(task["goal"], np.float32)
    Q = np.asarray(task["Q"], np.float32)
    if not task.get("diag", False):
        Q = Q.reshape(s, s)
    masses = o.plant_mass or [None]
    grid = [g for _ in masses for g in itertools.product(o.lams, o.upsilons, o.gammas, o.noises)]  # the grid once per plant mass
    n = len(grid)
    plant_of = [pm for pm in masses for _ in range(n // len(masses))]
    hb = m.BatchHandle(n=n, k=o.samples or conf["samples"], tau=conf["horizon"], s_dim=s, a_dim=a, dt=dt, mass=mass, goal=goal, Q=Q,
                       action_cost=m.ACTION_COST_PY, upsilon_scales_noise=True, seeds=[o.seed] * n,
                       lams=[g[0] for g in grid], upsilons=[g[1] for g in grid], gammas=[g[2] for g in grid],
                       sigmas=[g[3] * np.eye(a, dtype=np.float32) for g in grid])
    X = np.zeros((n, s), np.float32)
    t0 = time.perf_counter()
    plants = {pm: m.Handle(k=1, tau=1, s_dim=s, a_dim=a, dt=dt, mass=pm) for pm in masses if pm is not None}  # only their model is used
    ess_cols = None
    if o.on_device:
        Xs, _, _, st = hb.run_episode(X, o.steps, plant=[plants[pm] for pm in plant_of] if plants else None, stats=True)
        X = Xs[-1]
        ess_cols = (st.ess.mean(axis=0) / st.k, (st.ess < 2.0).mean(axis=0))  # per grid point, over the steps
    else:
        for _ in range(o.steps):
            X = plant(X, hb.next(X), dt, mass)
    wall = time.perf_counter() - t0
    dist = np.linalg.norm(X[:, 0::2] - goal[0::2], axis=1)
    mass_col = (lambda pm: " %10.3g" % pm) if plants else (lambda pm: "")
    print("%8s %8s %8s %8s%s  %s%s" % ("lambda", "upsilon", "gamma", "noise", " plant mass" if plants else "", "final goal distance",
                                      "    ess/K   needle" if ess_cols else ""))
    for i, ((lam, ups, gam, noise), pm, d) in enumerate(zip(grid, plant_of, dist)):
        print("%8.3g %8.3g %8.3g %8.3g%s  %.4f%s" % (lam, ups, gam, noise, mass_col(pm), d,
                                                    "%22.4f %8.2f" % (ess_cols[0][i], ess_cols[1][i]) if ess_cols else ""))
    best = int(np.argmin(dist))
    print("%d grid points, %d steps in one batch: %.2f s (%.1f us per batched step); best: lambda %.3g upsilon %.3g gamma %.3g noise %.3g%s "
          "(%.4f)" % (n, o.steps, wall, wall / max(o.steps, 1) * 1e6, *grid[best], (" on plant mass %.3g" % plant_of[best]) if plants else "",
                      dist[best]))
    if plants:  # which setting survives every vehicle: the grid point whose WORST plant ends nearest the goal
        worst = dist.reshape(len(masses), -1).max(axis=0)
        b = int(np.argmin(worst))
        print("most robust over plant masses %s: lambda %.3g upsilon %.3g gamma %.3g noise %.3g (worst final distance %.4f)" % (
            ",".join("%g" % pm for pm in masses), *grid[b], worst[b]))
    for p in plants.values():
        p.close()
    hb.close()


if __name__ == "__main__":
    main()
