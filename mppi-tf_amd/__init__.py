"""mppi-tf_amd — the MI355X-native MPPI control step behind the reference's plugin surface.

Scope: ONE hot path of NicolayP/mppi-tf: perturb K control sequences, roll the
model H steps, cost every step, soft-min weight, reduce to the new nominal sequence — as
hand-written HIP for gfx950 in csrc/, reached through the C-ABI of include/mppi_c.h.

  csrc/            HIP kernels + the C-ABI implementation  -> libmppi_hip.so (build.py)
  _lib.py          ctypes binding (Handle; BatchHandle: B controllers stepped together)
  controller.py    the reference's ControllerBase / StaticCost / PointMassModel interface; NNPointMassModel, the learned point mass
  auv.py           the 13-state family: AUVModel, NNAUVModel, NNAUVModelSpeed, StaticQuatCost, ElipseCost3D
  learner.py       LearnerBase: replay buffer + full-batch Adam on the GPU (csrc/mppi_learner.hip, mppi_learner_wide.hip) -> the learned model's weights;
                   k_fold_validation / grid_search on a LearnerBatch (csrc/mppi_learner_batch.hip: B learners in the launches of one) or, for
                   the [in, 256, 256, out] network, a WideLearnerBatch (csrc/mppi_learner_wide_batch.hip)
  distributed.py   K-sharding across GPUs (one process per GPU, one all-gather per step)
"""
from . import build as _build  # noqa: F401
from ._lib import (ACTION_COST_CPP, ACTION_COST_PY, CSV_REFERENCE, CSV_ROUNDTRIP, DBG_AUX, DBG_BETA, DBG_COSTS, DBG_ETA, DBG_NOISE,
                   DBG_U_UPDATED, DBG_WEIGHTS, BatchHandle, Handle, MppiError, StepStats, load)
from .controller import ControllerBase, ControllerBaseCpp, CostBase, ElipseCost, NNPointMassModel, PointMassModel, StaticCost
from .auv import AUVModel, ElipseCost3D, NNAUVModel, NNAUVModelSpeed, StaticQuatCost
from .learner import LearnerBase, kfold_indices
from ._lib import Learner, LearnerBatch, WideLearnerBatch

__all__ = ["Handle", "BatchHandle", "StepStats", "MppiError", "load", "ControllerBase", "ControllerBaseCpp", "CostBase", "PointMassModel", "NNPointMassModel",
           "StaticCost", "ElipseCost", "AUVModel", "NNAUVModel", "NNAUVModelSpeed", "StaticQuatCost", "ElipseCost3D", "LearnerBase", "Learner", "LearnerBatch", "WideLearnerBatch", "kfold_indices", "ACTION_COST_CPP", "ACTION_COST_PY", "DBG_COSTS", "DBG_BETA", "DBG_ETA", "DBG_WEIGHTS",
           "DBG_NOISE", "DBG_U_UPDATED", "DBG_AUX", "CSV_REFERENCE", "CSV_ROUNDTRIP"]
