"""Host-side mirror of the reference's learner for the learned model_base:
scripts/src/learners/learner_base.py LearnerBase — replay buffer, normalisation statistics, train_all / train / _train_step.

Same method names and argument meaning. What is numeric — the network's forward pass, the loss, the gradients and the Adam
update — runs on the GPU (mppi_learner.hip through the C-ABI's mppi_learner_*); the bookkeeping around it (replay buffer,
mean / std of the data, noise augmentation of the inputs) is numpy on the host, as it is host-side Python in the reference.
The reference's replay buffer is cpprb's ReplayBuffer (a ring of transitions): restated here as three numpy arrays.
k_fold_validation / grid_search (learner_base.py:83-216) train their k x R copies of the network as ONE LearnerBatch: every copy steps
in the same launches (mppi_learner_batch.hip), and validate_fold rolls every copy along held-out trajectories in one more
(mppi_learner_rollout.hip). A model whose network is [in, 256, 256, out] trains its copies as ONE WideLearnerBatch
(mppi_learner_wide_batch.hip) instead, rolled by WideLearnerBatch.validate (mppi_learner_wide_rollout.hip): k_fold_trajectory_validation
serves both families; k_fold_validation / grid_search keep refusing val= / episode= for a wide model.
TensorBoard logging and plotting are outside the path.
"""
import os

import numpy as np

from ._lib import Learner, LearnerBatch, WideLearnerBatch


def kfold_indices(n, k, seed=0):
    """k (train_idx, test_idx) pairs over range(n): one permutation split into k folds, the first n % k one row longer
    (sklearn.model_selection.KFold's fold sizes); fold i is test set i, the other folds in fold order are its training rows."""
    n, k = int(n), int(k)
    if k < 2 or k > n:
        raise ValueError("kfold_indices: 2 <= k <= n (k = %d, n = %d)" % (k, n))
    folds = np.array_split(np.random.default_rng(seed).permutation(n), k)
    return [(np.concatenate([folds[j] for j in range(k) if j != i]), folds[i]) for i in range(k)]


class ReplayBuffer:
    """a ring of (obs, act, next_obs) transitions (cpprb.ReplayBuffer's surface as learner_base.py:32-63 uses it)"""

    def __init__(self, size, sDim, aDim):
        self.size, self.n, self.head = int(size), 0, 0
        self.obs, self.act, self.next_obs = (np.zeros((self.size, d, 1)) for d in (sDim, aDim, sDim))

    def add(self, obs, act, next_obs):
        obs, act, next_obs = (np.asarray(v, np.float64) for v in (obs, act, next_obs))
        if obs.ndim == 2:
            obs, act, next_obs = obs[None], act[None], next_obs[None]
        for o, a, n in zip(obs, act, next_obs):
            self.obs[self.head], self.act[self.head], self.next_obs[self.head] = o, a, n
            self.head = (self.head + 1) % self.size
            self.n = min(self.n + 1, self.size)

    def get_all_transitions(self):
        return dict(obs=self.obs[:self.n], act=self.act[:self.n], next_obs=self.next_obs[:self.n])

    def save_transitions(self, filename):
        np.savez(filename, **self.get_all_transitions())

    def load_transitions(self, filename):
        d = np.load(filename)
        self.add(d["obs"], d["act"], d["next_obs"])


class Adam:
    """the hyper-parameters of tf.optimizers.Adam (learner_base.py:31, :149); the state lives on the device"""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon


class LearnerBase:
    def __init__(self, model, filename=None, bufferSize=264, numEpochs=100, batchSize=30, log=False, logPath=None, device=0):
        self.model = model
        self.sDim, self.aDim = model.get_state_dim(), model.get_action_dim()
        self.optimizer = Adam(learning_rate=0.5)  # learner_base.py:31
        self.rb = ReplayBuffer(bufferSize, self.sDim, self.aDim)
        self.numEpochs, self.batchSize = numEpochs, batchSize
        if filename is not None:
            self.load_rb(filename)
        self.log, self.step, self.sigma = log, 0, 0.001
        self._device, self._dev, self._dev_model = device, None, None
        self.last_losses = []
        self.logdir = logPath  # where save_params puts weights_step<N> (learner_base.py:40-52 stamps a sub-directory; this keeps the path given)
        self.val_log = []      # (epoch, validate(...)) of the last train(..., val=...)
        self.kfold_log = None  # dict(train, test [epoch, R, k][, val [ceil(epoch / 10), R, k]]) of the last k_fold_validation

    # ---- replay buffer (learner_base.py:54-66)
    def load_rb(self, filename):
        self.rb.load_transitions(filename)

    def add_rb(self, x, u, xNext):
        self.rb.add(obs=x, act=u, next_obs=xNext)

    def rb_trans(self):
        return {k: v.copy() for k, v in self.rb.get_all_transitions().items()}

    def save_rb(self, filename):
        self.rb.save_transitions(filename)

    # ---- persistence (learner_base.py:66-68 save_params -> NNModel.save_params, nn_model.py:137-142). The reference saves the
    # Keras model only; this file also carries both Adam moments and the step count (mppi_learner_save's flat format), so that a
    # run resumed in a new process continues bit for bit.
    def params_path(self, step, logdir=None):
        return os.path.join(logdir or self.logdir or ".", "weights_step{}".format(step))

    def save_params(self, step, logdir=None):
        path = self.params_path(step, logdir)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        self._device_learner(self.model).save(path, self.model.normalisation())
        return path

    def load_params(self, path):
        """weights + normalisation into the model, weights + Adam moments + step count into the device learner"""
        self._dev, norm = Learner.from_file(path, device=self._device)
        self._dev_model = self.model
        self._pull(self.model)
        if norm is not None:
            self.model.set_Xmean_Xstd(norm["xmean"], norm["xstd"])
            self.model.set_Ymean_Ystd(norm["ymean"], norm["ystd"])
        self.step = self._dev.step_count()

    def stats(self):
        """mean / std of the un-normalised training pairs become the model's normalisation (learner_base.py:71-83)"""
        data = self.rb_trans()
        X, y = self.model.prepare_training_data(data["obs"], data["next_obs"], data["act"], norm=False)
        std = lambda a: np.where(np.std(a, axis=0) > 0, np.std(a, axis=0), 1.0)  # a constant feature keeps its scale (the reference divides by 0)
        self.model.set_Xmean_Xstd(np.mean(X, axis=0), std(X))
        self.model.set_Ymean_Ystd(np.mean(y, axis=0), std(y))

    # ---- training (learner_base.py:146-153, 324-358, 469-496)
    def _device_learner(self, model):
        """The device learner holding `model`'s CURRENT weights. In the reference learner and model share tf.Variables, so
        model.update_weights(...) (the grid search's reset, learner_base.py:143; a loaded weight file) takes effect on the next
        step; here the weights are pushed before every train / evaluate — a few KB (they used to be uploaded once,
        at first use, and a later update_weights was silently ignored and then overwritten by _pull). The Adam moments stay, as
        an optimizer's slots do when its variables are assigned. One device learner per model object."""
        w = model.get_weights()
        weights = dict(W=w[0::2], b=w[1::2])
        if self._dev is None or self._dev_model is not model:
            self._dev, self._dev_model = Learner(weights, device=self._device), model
        else:
            self._dev.set_weights(weights)
        return self._dev

    def train_all(self, learningRate=0.1, batchSize=32, epoch=100, val=None, writer=None, augment=True):
        self.optimizer = Adam(learning_rate=learningRate)
        if self._dev is not None:
            self._dev.reset_optimizer()  # a new tf.optimizers.Adam (learner_base.py:149)
        data = self.rb_trans()
        X, y = self.model.prepare_training_data(data["obs"], data["next_obs"], data["act"])
        return self.train(X, y, epoch=epoch, learningRate=learningRate, val=val, writer=writer, augment=augment)

    def k_fold_validation(self, k=10, learningRate=0.1, batchSize=32, epoch=100, val=None, writer=None, seed=0, episode=None):
        """learner_base.py:83-127: k copies of the model, copy f trained on every fold but f and tested on fold f after each step, each with
        its own Adam. learningRate: one rate, or R of them (R x k copies: grid_search's rate axis). All copies are members of ONE
        LearnerBatch. -> dict(train=[epoch, R, k], test=[epoch, R, k]): the loss of each step's forward pass before its update, and of the
        updated weights on the held-out fold; kept in self.kfold_log, and handed epoch by epoch to `writer(e, dict(train=[R, k],
        test=[R, k]))`. The model and the object's own device learner are not touched (the reference trains copies). batchSize is accepted
        and ignored, as in train_all; the pairs are train_all's, without augmentation.
        val = (gtTrajs [kv, tau, s], actionSeqs [kv, tau, a]): after the step of every epoch e with e % 10 == 0 (learner_base.py:186-188)
        every copy is rolled along the held-out trajectories (validate_fold: one launch for all copies); the dict gains
        val=[ceil(epoch / 10), R, k] and the writer's dict of those epochs `val` [R, k]. The epochs then run in calls of 1, 10, 10, ... steps;
        train and test are the bits of a run without val."""
        if val is not None:
            self._check_val(val)
        if self.rb.n < 1:
            raise ValueError("k_fold_validation: the replay buffer holds no transitions")
        if self._is_wide(self.model.get_weights()) and (val is not None or episode is not None):
            raise ValueError("k_fold_validation: val= and episode= roll every member's network, and trajectory validation of wide members "
                             "is not built into this method: use k_fold_trajectory_validation ([in, 256, 256, out] trains and tests as a "
                             "WideLearnerBatch; choose by=\"test\")")
        return self._k_fold(k, learningRate, epoch, val, writer, seed, episode)

    def k_fold_trajectory_validation(self, k=10, learningRate=0.1, epoch=100, val=None, writer=None, seed=0):
        """k_fold_validation(val=) for every model, narrow or wide: k x R copies trained as ONE LearnerBatch or ONE WideLearnerBatch, the
        epochs in calls of 1, 10, 10, ... steps, and behind every epoch e with e % 10 == 0 every copy rolled along the held-out
        trajectories val = (gtTrajs [kv, tau, s], actionSeqs [kv, tau, a]) in one launch (validate_fold: LearnerBatch.rollout or
        WideLearnerBatch.validate) -> dict(train=[epoch, R, k], test=[epoch, R, k], val=[ceil(epoch / 10), R, k]), kept in self.kfold_log
        and handed to `writer` as k_fold_validation does. On a narrow model the bits of k_fold_validation(val=)."""
        self._check_val(val)
        if self.rb.n < 1:
            raise ValueError("k_fold_trajectory_validation: the replay buffer holds no transitions")
        return self._k_fold(k, learningRate, epoch, val, writer, seed, None)

    def _k_fold(self, k, learningRate, epoch, val, writer, seed, episode):
        """the body of k_fold_validation and k_fold_trajectory_validation (their arguments, checked)"""
        w = self.model.get_weights()
        wide = self._is_wide(w)
        rates = np.atleast_1d(np.asarray(learningRate, np.float32)).ravel()
        data = self.rb_trans()
        X, y = self.model.prepare_training_data(data["obs"], data["next_obs"], data["act"])
        folds = kfold_indices(len(X), k, seed)
        R, k = len(rates), len(folds)
        batch = (WideLearnerBatch if wide else LearnerBatch)(dict(W=w[0::2], b=w[1::2]), R * k, device=self._device)
        vals = []
        try:
            batch.set_data(X, y)
            for r in range(R):
                for f, (tr, te) in enumerate(folds):
                    batch.set_split(r * k + f, tr, te)
            if val is None:
                loss_train, loss_test = batch.train(epoch, np.repeat(rates, k))
            else:
                pieces, e = [], 0
                while e < epoch:  # epoch e = 0, then 1..10, 11..20, ...: a validation behind every epoch that is a multiple of 10
                    steps = 1 if e == 0 else min(10, epoch - e)
                    pieces.append(batch.train(steps, np.repeat(rates, k)))
                    e += steps
                    if (e - 1) % 10 == 0:
                        vals.append(self.validate_fold(batch, val).reshape(R, k))
                loss_train, loss_test = (np.concatenate([p[i] for p in pieces]) for i in (0, 1))
            # episode = episode_fold's keywords: every copy's closed-loop episode after the last epoch (grid_search by="episode")
            ep_cost = None if episode is None else self.episode_fold(batch, **episode)
        finally:
            batch.close()
        self.kfold_log = dict(train=loss_train.reshape(epoch, R, k), test=loss_test.reshape(epoch, R, k))
        if ep_cost is not None:
            self.kfold_log["episode"] = ep_cost.reshape(1, R, k)
        if val is not None:
            self.kfold_log["val"] = np.stack(vals)
        if callable(writer):
            for e in range(epoch):
                entry = dict(train=self.kfold_log["train"][e], test=self.kfold_log["test"][e])
                if val is not None and e % 10 == 0:
                    entry["val"] = self.kfold_log["val"][e // 10]
                writer(e, entry)
        return self.kfold_log

    @staticmethod
    def _is_wide(w):
        """is [W0, b0, W1, b1, ...] the [in, 256, 256, out] network (in, out <= 32) that a WideLearnerBatch trains?"""
        widths = [np.shape(w[0])[0]] + [np.shape(k)[1] for k in w[0::2]]
        return len(widths) == 4 and widths[1] == widths[2] == 256 and 1 <= widths[0] <= 32 and 1 <= widths[3] <= 32

    def _check_val(self, val):
        """val = (gtTrajs [kv, tau, s], actionSeqs [kv, tau, a]) with tau >= 2 -> the two arrays; ValueError before any device"""
        if not isinstance(val, (tuple, list)) or len(val) != 2:
            raise ValueError("val is (gtTrajs [k, tau, s], actionSeqs [k, tau, a])")
        gt, act = np.asarray(val[0]), np.asarray(val[1])
        if gt.ndim != 3 or act.ndim != 3 or gt.shape[:2] != act.shape[:2] or gt.shape[2] != self.sDim or act.shape[2] != self.aDim \
                or gt.shape[0] < 1 or gt.shape[1] < 2:
            raise ValueError("val is (gtTrajs [k, tau, %d], actionSeqs [k, tau, %d]) with k >= 1, tau >= 2, not %s and %s"
                             % (self.sDim, self.aDim, gt.shape, act.shape))
        return gt, act

    def validate_fold(self, batch, val, split=False, norm=False):
        """The multi-step error of every member of `batch` (learner_base.py:211-216 calls validate on each fold's model): each member's
        network, as this learner's model (its kind and normalisation), rolled tau - 1 steps from gtTrajs[:, 0] along actionSeqs, all
        members in ONE launch (LearnerBatch.rollout; WideLearnerBatch.validate for a wide batch) -> err [B] = sum of squared errors /
        (k tau s); the t = 0 term is zero and counts in the mean, as in validate (learner_base.py:264-267). split: also errSplit [B, s]. norm: behind each, its twin in the network's
        output units, sse / Ystd^2 (a model that normalises its last 6 outputs only, NNAUVModelSpeed: over those, as validate)."""
        gt, act = self._check_val(val)
        kv, tau, s = gt.shape
        roll = batch.rollout if hasattr(batch, "rollout") else batch.validate  # a LearnerBatch, or a WideLearnerBatch
        sse = roll(self.model, gt[:, 0], np.ascontiguousarray(np.swapaxes(act[:, :tau - 1], 0, 1)), gt=np.ascontiguousarray(np.swapaxes(gt, 0, 1)))["sse"]
        errSplit = sse / float(kv * tau)
        out = [errSplit.mean(axis=1)]
        ystd = np.asarray(self.model.Ystd, np.float64).ravel()
        errSplitNorm = errSplit[:, -len(ystd):] / ystd ** 2
        if norm:
            out.append(errSplitNorm.mean(axis=1))
        if split:
            out += [errSplit] + ([errSplitNorm] if norm else [])
        return out[0] if len(out) == 1 else tuple(out)

    def episode_fold(self, batch, controller, plant, x0, n_steps, goals=None):
        """What each member of `batch` is worth as a controller's model: every member's network, with this learner's model's normalisation,
        goes into the B learned controllers `controller` (BatchHandle.learned of B = batch.B members; load_learners), which then run ONE
        closed-loop episode of n_steps steps on the true vehicle `plant` (a Handle, or B of them) from x0 [s] or [B, s], from a zero sequence
        and step counter 0 -> the summed state cost of each member's episode, C.sum(0), [B]. goals: [n_steps, s] or [n_steps, B, s].
        `batch` is a LearnerBatch or a WideLearnerBatch: for an NNPointMassModel, narrow or wide, `controller` is
        BatchHandle.learned(B, ..., model="mlp", a_dim=). k_fold_validation(episode=) and grid_search(by="episode") reach this for narrow
        models only (they refuse a wide one); for the [in, 256, 256, out] network call episode_fold directly on the WideLearnerBatch."""
        B = batch.B
        controller.load_learners(batch, self.model)
        controller.set_action_sequences(np.zeros((B, controller.tau, controller.a), np.float32))
        controller.set_step_counter(0)
        x0 = np.asarray(x0, np.float32)
        X0 = np.ascontiguousarray(np.broadcast_to(x0, (B, controller.s)))
        if goals is not None:
            goals = np.asarray(goals, np.float32)
            goals = np.ascontiguousarray(np.broadcast_to(goals[:, None] if goals.ndim == 2 else goals, (int(n_steps), B, controller.s)))
        return controller.run_episode(X0, n_steps, goals, plant=plant)[2].sum(0)

    def grid_search(self, learningRates, k=2, epoch=250, seed=0, val=None, by="test", episode=None):
        """learner_base.py:129-216 without its TensorBoard writers and its sigma axis (augmented rows go into the pool by the caller's hand):
        every rate x every fold in one k_fold_validation -> (best_rate, table); by="test": table[r] = the mean over the folds of the last
        epoch's held-out loss; by="val" (needs val, k_fold_validation's): of the last validation's trajectory error; by="episode" (needs
        episode = dict(controller=, plant=, x0=, n_steps=[, goals=]), episode_fold's arguments; the controller has R * k members): of the
        summed state cost of each copy's closed-loop episode after the last epoch. best_rate is the table's argmin."""
        if by == "episode":
            if not isinstance(episode, dict) or not all(key in episode for key in ("controller", "plant", "x0", "n_steps")):
                raise ValueError('grid_search: by="episode" needs episode = dict(controller=, plant=, x0=, n_steps=[, goals=])')
        elif by not in ("test", "val") or (by == "val" and val is None):
            raise ValueError('grid_search: by is "test" or "val", and "val" needs val = (gtTrajs, actionSeqs)')
        rates = [float(r) for r in np.atleast_1d(learningRates).ravel()]
        log = self.k_fold_validation(k=k, learningRate=rates, epoch=epoch, seed=seed, val=val, episode=episode if by == "episode" else None)
        table = log[by][-1].astype(np.float64).mean(axis=1)
        return rates[int(np.argmin(table))], table

    def augment_data(self, X, y, samples=5, sigma=0.001, seed=1):
        """every pair `samples` times with N(0, sigma) noise on the inputs (learner_base.py:446-466). The reference then passes the
        DE-normalised arrays to a step that expects normalised ones (:464-465, a no-op at identity statistics): not reproduced —
        the network is trained on the normalised pairs it will be evaluated on."""
        XAug, yAug = np.repeat(X, samples, axis=0), np.repeat(y, samples, axis=0)
        return XAug + np.random.default_rng(seed).normal(0.0, sigma, XAug.shape), yAug

    def train(self, X, y, epoch=1, learningRate=0.1, augment=False, val=None, writer=None):
        """`epoch` full-batch Adam steps. With augmentation the reference draws fresh input noise every epoch (learner_base.py:326-329,
        with the SAME seed every time: the same noise); here the augmented set is drawn once and stays on the device."""
        XEp, yEp = self.augment_data(X, y, sigma=self.sigma) if augment else (X, y)
        dev = self._device_learner(self.model)
        dev.set_data(XEp, yEp)
        o = self.optimizer
        self.val_log = []
        if val is None:
            first, last = dev.train(epoch, learningRate, o.beta_1, o.beta_2, o.epsilon)
        else:
            # learner_base.py:336-358: every 10th epoch the model is validated on held-out trajectories val = (gtTrajs, actionSeqs):
            # the epochs run on the device in blocks of 10 with the validation between them (the reference logs the numbers to
            # TensorBoard; they are kept in self.val_log and handed to `writer(epoch, dict)` if one is given)
            first = last = None
            for e0 in range(0, epoch, 10):
                self._pull(self.model)
                errs = self.validate(self.model, val[1], val[0], transition=True, split=True, norm=True)
                names = ("Val-Total", "Val-Total-Norm", "Val-Split", "Val-Split-Norm", "Val-Transition", "Val-Transition-Norm",
                         "Val-Transition-Split", "Val-Transition-Split-Norm")
                entry = dict(zip(names, errs))
                self.val_log.append((e0, entry))
                if callable(writer):
                    writer(e0, entry)
                f, last = dev.train(min(10, epoch - e0), learningRate, o.beta_1, o.beta_2, o.epsilon)
                first = f if first is None else first
        self.last_losses = [first, last]
        self._pull(self.model)
        self.step += epoch
        return first, last

    # ---- validation (learner_base.py:218-320)
    def norm_trajs(self, model, trajs):
        """trajectories [k, tau, s] in the network's output units (learner_base.py:360-367: (traj - Ymean) / Ystd)"""
        return (np.asarray(trajs, np.float64) - np.asarray(model.Ymean)) / np.asarray(model.Ystd)

    def validate(self, model, actionSeqs, gtTrajs, plot=False, transition=False, split=False, norm=False):
        """Error of the model on k trajectories gtTrajs [k, tau, s] with their action sequences actionSeqs [k, tau, a]
        (learner_base.py:218-320): the model is rolled tau-1 steps from each trajectory's first state (on the device, the model's own
        step) and compared with the ground truth — err [, errNorm] [, errSplit, errSplitNorm] — and with transition=True every
        (x_t, u_t) -> x_t+1 pair is predicted on its own (transErr...). Same return tuples as the reference for every flag combination."""
        actionSeqs, gtTrajs = np.asarray(actionSeqs, np.float64), np.asarray(gtTrajs, np.float64)
        tau = actionSeqs.shape[1]
        state = gtTrajs[:, 0][..., None]
        trajs = [state[:, None]]
        for i in range(tau - 1):
            state = np.asarray(model.build_step_graph("val", state, actionSeqs[:, i][..., None]), np.float64)
            trajs.append(state[:, None])
        trajs = np.concatenate(trajs, axis=1)[..., 0]
        errSplit = np.mean((trajs - gtTrajs) ** 2, axis=(0, 1))
        err = float(np.mean(errSplit))
        out_n = len(np.asarray(model.Ymean).ravel())
        if out_n == trajs.shape[-1]:
            errSplitNorm = np.mean((self.norm_trajs(model, trajs) - self.norm_trajs(model, gtTrajs)) ** 2, axis=(0, 1))
        else:  # NNAUVModelSpeed normalises the 6 velocity outputs only: its trajectory error in those units (state[7:13])
            errSplitNorm = np.mean(((trajs[..., -out_n:] - gtTrajs[..., -out_n:]) / np.asarray(model.Ystd)) ** 2, axis=(0, 1))
        errNorm = float(np.mean(errSplitNorm))
        if transition:
            k, s_dim, a_dim = gtTrajs.shape[0], gtTrajs.shape[2], actionSeqs.shape[2]
            actions = actionSeqs[:, :-1].reshape((tau - 1) * k, a_dim, 1)
            states = gtTrajs[:, :-1].reshape((tau - 1) * k, s_dim, 1)
            nextStates = gtTrajs[:, 1:].reshape((tau - 1) * k, s_dim, 1)
            XNorm, yNorm = model.prepare_training_data(states, nextStates, actions)
            dev = Learner(dict(W=model.get_weights()[0::2], b=model.get_weights()[1::2]), device=self._device)  # the network alone (model._predict_nn)
            dev.set_data(XNorm, yNorm)
            _, predNorm = dev.evaluate(pred=True)
            dev.close()
            yN = np.asarray(yNorm, np.float32)
            transErrSplitNorm = np.mean((predNorm - yN) ** 2, axis=0)
            transErrNorm = float(np.mean(transErrSplitNorm))
            transErrSplit = np.mean(((predNorm - yN) * np.asarray(model.Ystd)) ** 2, axis=0)  # denormalizeY: Ymean cancels in the difference
            transErr = float(np.mean(transErrSplit))
        # What the caller unpacks (learner_base.py:301-322), built instead of enumerated: the trajectory error, then with `norm` its normalised
        # twin, then with `split` the per-dimension pair; with `transition` the same pattern again for the one-step error.
        def pattern(e, eNorm, eSplit, eSplitNorm):
            out = [e] + ([eNorm] if norm else [])
            if split:
                out += [eSplit] + ([eSplitNorm] if norm else [])
            return out

        out = pattern(err, errNorm, errSplit, errSplitNorm)
        if transition:
            out += pattern(transErr, transErrNorm, transErrSplit, transErrSplitNorm)
        return out[0] if len(out) == 1 else tuple(out)

    def _train_step(self, model, optimizer, Xnorm, Ynorm, split=False, norm=False):
        """ONE Adam step on (Xnorm, Ynorm) (learner_base.py:469-496) -> (loss, grads): the loss of the forward pass before the update in
        normalised AND de-normalised units is the same number at identity statistics; returned as (loss, lossNorm, grads) with norm=True."""
        dev = self._device_learner(model)
        dev.set_data(Xnorm, Ynorm)
        lossNorm, grads, pred = dev.evaluate(grads=True, pred=True)
        dev.train(1, optimizer.learning_rate, optimizer.beta_1, optimizer.beta_2, optimizer.epsilon)
        self._pull(model)
        # the de-normalised loss (learner_base.py:482-486): Ymean cancels in the difference, Ystd scales it
        loss = float(np.mean(((pred - np.asarray(Ynorm, np.float32)) * np.asarray(model.Ystd, np.float64)) ** 2))
        glist = []
        for w, b in zip(grads["W"], grads["b"]):
            glist += [w, b]
        if norm:
            return loss, lossNorm, glist
        return loss, glist

    def evaluate(self, model, X, y):
        dev = self._device_learner(model)
        dev.set_data(X, y)
        return dev.evaluate()

    def _pull(self, model):
        w = self._dev.get_weights()
        flat = []
        for W, b in zip(w["W"], w["b"]):
            flat += [W, b]
        model.update_weights(flat, msg=False)
