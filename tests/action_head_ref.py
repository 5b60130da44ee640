"""Plain-torch restatement of the deterministic policy's output head and losses: the reference's ``ICLTransformer``
(robomimic/algo/icl.py:41-75 builds it when ``algo.gmm.enabled`` is False, config/icl_config.py:63) -- the ObservationDecoder's one
Linear ``action`` (robomimic/models/obs_nets.py:763-771 with the output shape of policy_nets.py:1683-1690), ``tanh``
(policy_nets.py:1728-1731) and ``ICL._compute_losses`` (icl.py:174-202) with ``LossUtils.cosine_loss`` (utils/loss_utils.py:11-23)
-- as functions of a ``state_dict``, in the style of tests/gmm_ref.py: it issues the reference's own ops (``F.linear``,
``torch.tanh``, ``nn.MSELoss``, ``nn.SmoothL1Loss``, ``nn.CosineSimilarity``, the weighted ``sum``), runs on any device and in any
float dtype (the float64 yardstick of tests/test_gpu_action_head.py is this code on ``.double()`` CPU tensors), and
scripts/bench_action_head.py times it as the eager baseline.
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

KEYS = ("nets.action.weight", "nets.action.bias")
LOSS_KEYS = ("l2_loss", "l1_loss", "cos_loss", "action_loss")
DEFAULT_WEIGHTS = (1.0, 0.0, 0.0)         # icl_config.py:43-45: l2_weight, l1_weight, cos_weight


def decoder(sd, feats, prefix="nets."):
    """obs_nets.py:763-771: the raw `action` output [..., A] of feats [..., E]."""
    return F.linear(feats, sd[prefix + "action.weight"], sd[prefix + "action.bias"])


def actions(sd, feats):
    """policy_nets.py:1728-1731: tanh of the decoder's output."""
    return torch.tanh(decoder(sd, feats))


def cosine_loss(preds, labels):
    """utils/loss_utils.py:11-23."""
    sim = nn.CosineSimilarity(dim=len(preds.shape) - 1)(preds, labels)
    return -torch.mean(sim - 1.0)


def compute_losses(acts, target, weights=DEFAULT_WEIGHTS):
    """icl.py:187-202 on predicted actions and their targets [..., A]."""
    losses = OrderedDict()
    losses["l2_loss"] = nn.MSELoss()(acts, target)
    losses["l1_loss"] = nn.SmoothL1Loss()(acts, target)
    losses["cos_loss"] = cosine_loss(acts[..., :3], target[..., :3])
    action_losses = [weights[0] * losses["l2_loss"], weights[1] * losses["l1_loss"], weights[2] * losses["cos_loss"]]
    losses["action_loss"] = sum(action_losses)
    return losses


def head_losses(sd, feats, target, weights=DEFAULT_WEIGHTS):
    return compute_losses(actions(sd, feats), target, weights)
