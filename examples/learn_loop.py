#!/usr/bin/env python3
"""The reference's experiment as one script: a controller whose model is LEARNED (NNAUVModel, examples/config/auv_nn_model.yaml: Dense(32)
x 3 + Dense(13), random initial weights) drives the true vehicle (the rexrov2 Fossen model), logs every transition, trains on them and
takes the new weights — round after round. A round's control steps run on the device as ONE call, run_episode(..., plant=fossen): the
controller plans with its network, the state is stepped by the Fossen plant handle, no host round trip between the steps.
    python examples/learn_loop.py                                             # 4 rounds of 50 steps, K = 1024, H = 20, 100 epochs
    python examples/learn_loop.py --rounds 2 --samples 128 --horizon 8 --steps 8 --epochs 3 --hidden 16 --layers 1
Each round: run_episode from x0 -> every (X[t], U[t], X[t+1]) into LearnerBase.add_rb -> statistics, train_all on the whole buffer ->
the new weights and normalisation into the controller (Handle.set_mlp, the mppi_set_mlp path). Each round prints the mean state cost of
its episode, the one-step error of the model on that round's transitions and its H-step OPEN-LOOP error — what an MPPI controller needs
from its model, because its rollouts are H steps long — each before and after the training. The H-step error takes every window
x0 = X[t], V = U[t:t+H] of the round's episode and rolls it twice, once on the controller's handle (the learned model) and once on the
Fossen plant handle (the truth), each as ONE model_rollout call over all windows; the figure is the mean distance between the two
positions at step H. The script makes no claim about convergence: it shows the loop, and the numbers say what the rounds did.
    python examples/learn_loop.py --model point_mass --hidden 256
is the same loop for the point mass: the controller's model is NNPointMassModel (MPPI_MODEL_MLP; --hidden 256: Dense(256) x 2, the network
of the matrix-core rollout kernel, trained by the wide learner), the plant a k = 1, tau = 1 handle of the analytic point mass (2 actions,
state (x, vx, y, vy)); the H-step error takes the position components 0 and 2.
    python examples/learn_loop.py --kfold 5 --lrs 1e-3,3e-3,1e-2
chooses each round's learning rate first: LearnerBase.grid_search trains every rate x every fold as ONE batch of learners (LearnerBatch)
and the rate with the smallest mean held-out loss trains the model; one more line per round shows the table. With --model point_mass
--hidden 256 the batch is a WideLearnerBatch, the same held-out table for the [in, 256, 256, out] network.
    python examples/learn_loop.py --kfold 5 --lrs 1e-3,3e-3,1e-2 --kfold-val
chooses the rate by what the controller needs instead: every fold's network is rolled H steps open-loop along the windows of the round's
episode (LearnerBase.k_fold_trajectory_validation / validate_fold: all rates x folds in one launch, narrow networks and the --hidden 256
one alike) and the rate with the smallest mean H-step error wins; a second line per round shows that table.
    python examples/learn_loop.py --kfold 5 --lrs 1e-3,3e-3,1e-2 --kfold-episode
chooses the rate by what the model is FOR: every fold's network becomes the model of its own controller — rates x folds learned
controllers in one batch (BatchHandle.learned, one network per member, stepped in the same two launches as one) — and each runs a short
closed-loop episode on the Fossen plant from x0 (LearnerBase.episode_fold: --episode-steps steps, all members in one call); the rate with
the smallest mean summed state cost wins, and a second line per round shows that table."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mppi_tf_amd as m  # noqa: E402
from mppi_tf_amd.auv import auv_task  # noqa: E402


def glorot(dims, seed):
    """Keras' default initialisation of Dense layers: glorot-uniform kernels, zero biases"""
    rng = np.random.default_rng(seed)
    lim = [np.sqrt(6.0 / (dims[i] + dims[i + 1])) for i in range(len(dims) - 1)]
    return dict(W=[rng.uniform(-lim[i], lim[i], (dims[i], dims[i + 1])).astype(np.float32) for i in range(len(dims) - 1)],
                b=[np.zeros(dims[i + 1], np.float32) for i in range(len(dims) - 1)])


def one_step_error(model, X, U):
    """mean squared error of the model's one-step prediction on the transitions (X[t], U[t]) -> X[t+1]"""
    pred = np.asarray(model.predict(X[:-1, :, None], U[:, :, None]), np.float64)[..., 0]
    return float(np.mean((pred - X[1:]) ** 2))


def h_step_error(cont, plant, X, U, H, pos=(0, 1, 2)):
    """mean position error at step H of the controller's model rolled open-loop along the recorded actions, over every window
    x0 = X[t], V = U[t:t+H] of the episode, against the plant rolled along the same actions: two model_rollout calls. -> (error, windows)"""
    n = U.shape[0] - H + 1
    if n < 1:
        return float("nan"), 0
    V = np.ascontiguousarray(np.stack([U[t:t + H] for t in range(n)], axis=1))  # [H, n, a]
    Xm = cont.model_rollout(X[:n], V, costs=False)[0]
    Xp = plant.model_rollout(X[:n], V, costs=False)[0]
    pos = list(pos)
    return float(np.mean(np.linalg.norm(Xm[-1][:, pos].astype(np.float64) - Xp[-1][:, pos].astype(np.float64), axis=1))), n


def windows_val(X, U, H):
    """the episode's windows as LearnerBase's val = (gtTrajs [n, H+1, s], actionSeqs [n, H+1, a]): window t holds X[t..t+H] and U[t..t+H-1]
    (the last action row of a trajectory is never applied: zeros)"""
    n = U.shape[0] - H + 1
    gt = np.stack([X[t:t + H + 1] for t in range(n)])
    act = np.stack([np.concatenate([U[t:t + H], np.zeros((1, U.shape[1]), U.dtype)]) for t in range(n)])
    return gt, act


def run(o):
    """-> (the learner, the rounds' episodes [(X, U, C)], the rounds' printed figures [(mean cost, error before, error after, loss first,
    loss last[, H-step error before, H-step error after: when the episode holds a window of H steps])])"""
    if o.model == "point_mass":
        # 2 actions, state (x, vx, y, vy): from rest at the origin to (1, -1); the plant is the analytic point mass
        a, dt, pos = 2, 0.1, (0, 2)
        task = dict(tau=o.horizon, s_dim=2 * a, a_dim=a, dt=dt, lam=1.0, sigma=np.eye(a, dtype=np.float32), goal=[1.0, 0.0, -1.0, 0.0],
                    Q=np.array([10.0, 1.0, 10.0, 1.0], np.float32), seed=1)
        x0 = np.zeros(2 * a, np.float32)
        hidden = (256, 256) if o.hidden == 256 else (o.hidden,) * o.layers
        model = m.NNPointMassModel(stateDim=2 * a, actionDim=a, hidden=hidden, weights=glorot([3 * a, *hidden, 2 * a], o.seed), dt=dt)
        cont = m.Handle(k=o.samples, mlp=model.mlp(), **task)
        fossen = m.Handle(k=1, tau=1, s_dim=2 * a, a_dim=a, dt=dt, mass=1.0)  # the plant: only its model is used
    else:
        pos = (0, 1, 2)
        task = auv_task(o.horizon, learned=True)
        x0 = np.asarray(task.pop("x0"), np.float32)
        model = m.NNAUVModel(weights=glorot([16] + [o.hidden] * o.layers + [13], o.seed), dt=task["dt"])
        cont = m.Handle(k=o.samples, nnauv=model.mlp(), **task)
        fossen = m.Handle(k=1, tau=1, s_dim=13, a_dim=6, dt=task["dt"], sigma=np.eye(6, dtype=np.float32), goal=np.zeros(13, np.float32),
                          auv=auv_task(1)["auv"])  # the plant: a handle that runs no rollouts, only its model is used
    learner = m.LearnerBase(model, bufferSize=o.rounds * o.steps)
    episodes, figures = [], []
    by_episode = getattr(o, "kfold_episode", False)
    # rates x folds learned controllers, one network each: they share the task and the Philox key, so only the networks tell them apart
    # (the learned point mass: BatchHandle.learned(model="mlp"); its narrow networks only — grid_search refuses a wide model's episode=)
    kind = dict(model="mlp", a_dim=task["a_dim"]) if o.model == "point_mass" else dict(model="nnauv")
    folds_ctl = m.BatchHandle.learned(len(o.lrs) * o.kfold, model.mlp(), k=o.samples, seeds=[task["seed"]] * (len(o.lrs) * o.kfold), **kind,
                                      **{k: v for k, v in task.items() if k not in ("s_dim", "a_dim", "seed")}) if by_episode else None
    for r in range(o.rounds):
        X, U, Cs = cont.run_episode(x0, o.steps, plant=fossen)
        episodes.append((X, U, Cs))
        learner.add_rb(X[:-1, :, None], U[:, :, None], X[1:, :, None])
        before = one_step_error(model, X, U)
        h_before, windows = h_step_error(cont, fossen, X, U, o.horizon, pos)
        learner.stats()
        lr = o.lr
        if getattr(o, "kfold", 0):
            # the round's rate by k-fold cross-validation over --lrs: every rate x every fold trains at once, as one batch of learners
            by_val = getattr(o, "kfold_val", False)
            episode = dict(controller=folds_ctl, plant=fossen, x0=x0, n_steps=o.episode_steps) if by_episode else None
            if by_val:  # narrow or wide ([in, 256, 256, out]: grid_search(by="val") refuses it): the last validation's table and its argmin
                log = learner.k_fold_trajectory_validation(k=o.kfold, learningRate=o.lrs, epoch=o.epochs, val=windows_val(X, U, o.horizon))
                table = log["val"][-1].astype(np.float64).mean(axis=1)
                lr = o.lrs[int(np.argmin(table))]
            else:
                lr, table = learner.grid_search(o.lrs, k=o.kfold, epoch=o.epochs, by="episode" if by_episode else "test", episode=episode)
            held_out = learner.kfold_log["test"][-1].astype(np.float64).mean(axis=1)
            print("round %d: %d-fold held-out loss after %d epochs by learning rate: %s -> lr %g" % (
                r + 1, o.kfold, o.epochs, ", ".join("%g: %.6g" % (a, b) for a, b in zip(o.lrs, held_out)), lr), flush=True)
            if by_val:
                print("round %d: %d-fold H-step open-loop squared error (H = %d, %d windows) after %d epochs by learning rate: %s -> lr %g" % (
                    r + 1, o.kfold, o.horizon, windows, 10 * ((o.epochs - 1) // 10) + 1,
                    ", ".join("%g: %.6g" % (a, b) for a, b in zip(o.lrs, table)), lr), flush=True)
            if by_episode:
                print("round %d: %d-fold summed state cost of a %d-step closed-loop episode on the plant after %d epochs by learning rate: %s "
                      "-> lr %g" % (r + 1, o.kfold, o.episode_steps, o.epochs, ", ".join("%g: %.6g" % (a, b) for a, b in zip(o.lrs, table)), lr),
                      flush=True)
        first, last = learner.train_all(learningRate=lr, epoch=o.epochs)
        cont.set_mlp(model.mlp())
        after = one_step_error(model, X, U)
        h_after, _ = h_step_error(cont, fossen, X, U, o.horizon, pos)
        figures.append((float(np.mean(Cs)), before, after, first, last) + ((h_before, h_after) if windows else ()))
        h_text = ("%.6g -> %.6g m (%d windows)" % (h_before, h_after, windows)) if windows else "n/a (the episode is shorter than H)"
        print("round %d: %d steps, mean state cost %.6g, one-step error of the model on this round's transitions %.6g -> %.6g "
              "(%d transitions, %d epochs, normalised loss %.6g -> %.6g), H-step open-loop position error (H = %d) %s" % (
                  r + 1, o.steps, figures[-1][0], before, after, learner.rb.n, o.epochs, first, last, o.horizon, h_text), flush=True)
        if getattr(o, "on_round", None) is not None:
            o.on_round(r, cont, model, X, U)
    if folds_ctl is not None:
        folds_ctl.close()
    cont.close()
    fossen.close()
    return learner, episodes, figures


def main(argv=None, on_round=None):
    """on_round(round, controller handle, model, X, U): called at the end of every round, while the handles are alive"""
    ap = argparse.ArgumentParser(description="a learned controller on the true plant: episode, train, new weights, round after round")
    ap.add_argument("--model", default="auv", choices=("auv", "point_mass"), help="auv: NNAUVModel on the Fossen plant; point_mass: NNPointMassModel on the analytic point mass")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("-s", "--steps", type=int, default=50, help="control steps per round (one run_episode call)")
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=100, help="Adam steps per round on the whole replay buffer")
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--hidden", type=int, default=32, choices=(16, 32, 256), help="width of the hidden layers (256: point_mass only, two layers)")
    ap.add_argument("--layers", type=int, default=3, choices=(1, 2, 3), help="hidden layers")
    ap.add_argument("--seed", type=int, default=0, help="of the initial weights")
    ap.add_argument("--kfold", type=int, default=0, help="K >= 2: choose each round's learning rate among --lrs by K-fold cross-validation (LearnerBase.grid_search)")
    ap.add_argument("--lrs", type=lambda v: [float(x) for x in v.split(",")], default=None, help="a,b,c: the learning rates --kfold chooses from")
    ap.add_argument("--kfold-val", action="store_true", help="with --kfold: choose the rate by the folds' H-step open-loop error on the round's episode (LearnerBase.validate_fold)")
    ap.add_argument("--kfold-episode", action="store_true", help="with --kfold (--model auv, or point_mass at --hidden 16 / 32): choose the rate by a short closed-loop episode of every fold's network on the plant (LearnerBase.episode_fold)")
    ap.add_argument("--episode-steps", type=int, default=10, help="steps of the --kfold-episode episodes")
    o = ap.parse_args(argv)
    if o.kfold_episode and (not o.kfold or o.kfold_val or (o.model == "point_mass" and o.hidden == 256) or o.episode_steps < 1):
        ap.error("--kfold-episode goes with --kfold (not with --model point_mass --hidden 256: the wide network's folds have no episode "
                 "harness), not with --kfold-val, and needs --episode-steps >= 1")
    if o.kfold_val and (not o.kfold or o.steps < o.horizon):
        ap.error("--kfold-val goes with --kfold and needs --steps >= --horizon")
    if bool(o.kfold) != bool(o.lrs):
        ap.error("--kfold K and --lrs a,b,c go together")
    if o.kfold and (o.kfold < 2 or o.kfold > o.steps):
        ap.error("--kfold: 2 <= K <= --steps")
    if o.hidden == 256 and o.model != "point_mass":
        ap.error("--hidden 256 is the point-mass network: use --model point_mass")
    o.on_round = on_round
    return run(o)


if __name__ == "__main__":
    main()
