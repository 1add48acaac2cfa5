"""The classification losses of the reference, under its registry names and constructor signatures so that config dicts
(``loss_cls=dict(type='CrossEntropyLoss', class_weight=[...])``) build unchanged
(pyskl/models/losses/cross_entropy_loss.py:11-123, scaled by ``loss_weight`` as base.py:38-44):

* ``CrossEntropyLoss``: ``(N,)`` integer labels -> ``F.cross_entropy`` (mean over the batch; with ``class_weight`` the
  weighted mean); ``(N, classes)`` float labels (soft labels) -> ``-sum_k q_k w_k log p_k`` per clip, averaged over the
  clips or, with ``class_weight``, divided by ``sum q_k w_k``.
* ``BCELossWithLogits``: ``(N, classes)`` float labels -> ``F.binary_cross_entropy_with_logits`` (mean over all
  elements, ``class_weight`` as its ``weight``).

These modules are plain torch on whatever device the scores are on: the path of heads with dropout and of CPU runs.  The
training step of a head without dropout does not call them: ``SimpleHead.forward_loss`` reads ``loss_weight`` and
``class_weight`` and runs head and loss as HIP kernels (``kernels.head_loss`` / ``kernels.head_target``).
``class_weight`` is a non-persistent buffer: it follows ``.to(device)`` and stays out of the state_dict, whose keys are
the reference's.  Extra ``F.cross_entropy`` kwargs are rejected."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .builder import LOSSES


class _WeightedLoss(nn.Module):

    def __init__(self, loss_weight=1.0, class_weight=None):
        super().__init__()
        self.loss_weight = float(loss_weight)
        cw = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float32).reshape(-1).clone()
        self.register_buffer('class_weight', cw, persistent=False)

    def _weight(self, cls_score):
        cw = self.class_weight
        if cw is None:
            return None
        if cw.numel() != cls_score.shape[1]:
            raise ValueError(f'{type(self).__name__}: {cw.numel()} class weights for {cls_score.shape[1]} classes')
        return cw.to(device=cls_score.device, dtype=cls_score.dtype)

    def _scaled(self, loss):
        return loss if self.loss_weight == 1.0 else loss * self.loss_weight


@LOSSES.register_module()
class CrossEntropyLoss(_WeightedLoss):

    def forward(self, cls_score, label):
        if cls_score.dim() != 2:
            raise NotImplementedError(f'CrossEntropyLoss: expects (N, classes) scores, got {tuple(cls_score.shape)}')
        cw = self._weight(cls_score)
        if cls_score.shape == label.shape and label.is_floating_point():
            lsm = F.log_softmax(cls_score, 1)
            if cw is None:
                return self._scaled(-(label * lsm).sum(1).mean())
            return self._scaled(-(label * (lsm * cw[None])).sum(1).sum() / (cw[None] * label).sum())
        if label.shape != cls_score.shape[:1] or label.is_floating_point():
            raise NotImplementedError(
                f'CrossEntropyLoss: expects (N, classes) scores with (N,) integer labels or (N, classes) float labels, got '
                f'{tuple(cls_score.shape)} / {tuple(label.shape)} {label.dtype}')
        return self._scaled(F.cross_entropy(cls_score, label, weight=cw))


@LOSSES.register_module()
class BCELossWithLogits(_WeightedLoss):

    def forward(self, cls_score, label):
        if cls_score.dim() != 2 or label.shape != cls_score.shape or not label.is_floating_point():
            raise NotImplementedError(
                f'BCELossWithLogits: expects (N, classes) scores with (N, classes) float labels, got '
                f'{tuple(cls_score.shape)} / {tuple(label.shape)} {label.dtype}')
        return self._scaled(F.binary_cross_entropy_with_logits(cls_score, label, weight=self._weight(cls_score)))
