"""Classification head of the skeleton recognizers, behind the reference's registry names ``GCNHead`` /
``SimpleHead`` and constructor kwargs (pyskl/models/heads/simple_head.py:12-140, heads/base.py:11-84).

What the path computes: global average over (T, V), mean over the M persons, ``Linear(in_channels, classes)``;
``loss()`` = the configured loss + top-1 / top-5 accuracy as log scalars.  Two deliberate differences from the
reference's host code: (i) the ranking runs on the device (one small ``topk``) instead of a device->host copy and a
numpy argsort per step (heads/base.py:67-72 syncs every iteration); the numbers are the same, ties aside; (ii) the
2D/3D pooling modes and list inputs are not reached by any skeleton config and are rejected rather than carried along;
(iii) ``forward_loss`` is the fused form of ``loss(forward(x), label)`` that ``RecognizerGCN.forward_train`` calls (the
two methods stay for everything else).

``multi_class`` / ``label_smooth_eps`` follow heads/base.py:60-77: a label of the scores' shape (soft or multi-hot) gets
no accuracies, smoothing applies only to a ``multi_class`` head, and the ``(classes,)`` label of a single clip is
unsqueezed."""
import torch
import torch.nn as nn

from . import kernels
from .builder import HEADS, build_loss


@HEADS.register_module()
class SimpleHead(nn.Module):

    def __init__(self, num_classes, in_channels, loss_cls=dict(type='CrossEntropyLoss'), dropout=0.5, init_std=0.01,
                 mode='3D', multi_class=False, label_smooth_eps=0.0):
        super().__init__()
        assert mode in ['3D', 'GCN', '2D']
        if mode != 'GCN':
            raise NotImplementedError('only the skeleton (GCN) pooling mode is on this path')
        self.num_classes = num_classes
        self.in_channels = self.in_c = in_channels
        self.mode = mode
        self.multi_class = bool(multi_class)
        self.label_smooth_eps = float(label_smooth_eps)
        self.loss_cls = build_loss(loss_cls)
        self.dropout_ratio = dropout
        self.init_std = init_std
        self.dropout = nn.Dropout(p=dropout) if dropout != 0 else None
        self.fc_cls = nn.Linear(in_channels, num_classes)

    def init_weights(self):
        nn.init.normal_(self.fc_cls.weight, 0, self.init_std)
        nn.init.constant_(self.fc_cls.bias, 0)

    def forward(self, x):
        """x (N, M, C, T, V) backbone features (or their plane means (N, M, C), or pooled (N, C)) -> scores (N, classes)."""
        if x.dim() == 5:
            N, M, C = x.shape[:3]
            x = x.reshape(N * M, C, -1).mean(-1).reshape(N, M, C).mean(1)
        elif x.dim() == 3:                          # per-person plane means from ``backbone(x, pool=True)``
            x = x.mean(1)
        elif x.dim() != 2:
            raise NotImplementedError(f'GCN head expects (N, M, C, T, V), (N, M, C) or (N, C) features, got {tuple(x.shape)}')
        assert x.shape[1] == self.in_c
        if self.dropout is not None:
            x = self.dropout(x)
        return self.fc_cls(x)

    def _prepare_label(self, label, clips):
        """heads/base.py:60-77 up to the loss call -> (label, whether the accuracies are reported)."""
        if label.dim() == 0:
            label = label[None]
        elif label.dim() == 1 and label.shape[0] == self.num_classes and clips == 1:
            label = label[None]
        same = label.dim() == 2 and tuple(label.shape) == (clips, self.num_classes)
        if self.multi_class and self.label_smooth_eps != 0:
            label = (1 - self.label_smooth_eps) * label + self.label_smooth_eps / self.num_classes
        return label, not self.multi_class and not same

    def forward_loss(self, x, label):
        """``loss(forward(x), label)`` as the training step runs it: person mean, ``fc_cls``, the loss and (for hard
        labels) both accuracies in three launches instead of ~25.  ``CrossEntropyLoss`` without class weights on integer
        labels is ``kernels.head_loss``; with class weights, on ``(N, classes)`` float labels, and ``BCELossWithLogits``
        are ``kernels.head_target`` modes 0 / 1 / 2.  Heads with dropout or another loss take the two calls."""
        from .losses import BCELossWithLogits, CrossEntropyLoss
        kind = type(self.loss_cls)
        if (not kernels.FUSED_ENDS or x.dim() not in (3, 5) or self.dropout is not None
                or kind not in (CrossEntropyLoss, BCELossWithLogits)):
            return self.loss(self(x), label)
        N, M, C = x.shape[:3]
        assert C == self.in_c
        label, with_acc = self._prepare_label(label, N)
        soft = label.is_floating_point() and tuple(label.shape) == (N, self.num_classes)
        cw, lw = self.loss_cls.class_weight, self.loss_cls.loss_weight
        if kind is BCELossWithLogits:
            if not soft:
                raise NotImplementedError(f'BCELossWithLogits: expects ({N}, {self.num_classes}) float labels, got '
                                          f'{tuple(label.shape)} {label.dtype}')
            mode = 2
        elif soft:
            mode = 1
        elif label.is_floating_point() or label.shape != (N,):
            raise NotImplementedError(f'CrossEntropyLoss: expects (N,) integer labels or (N, classes) float labels for '
                                      f'(N, classes) scores, got {tuple(label.shape)} {label.dtype} for {N} clips')
        else:
            mode = 0
        feat = x.reshape(N * M, C, -1).mean(-1) if x.dim() == 5 else x.reshape(N * M, C)
        if mode == 0 and cw is None:
            loss, acc, _ = kernels.ops().head_loss(feat, self.fc_cls.weight, self.fc_cls.bias, label, M, lw)
        else:
            loss, acc, _ = kernels.ops().head_target(feat, self.fc_cls.weight, self.fc_cls.bias, label, M, mode, cw, lw)
        if mode == 0 and with_acc:
            return dict(top1_acc=acc[0], top5_acc=acc[1], loss_cls=loss)
        return dict(loss_cls=loss)

    def loss(self, cls_score, label):
        """-> dict(loss_cls) + (for labels of another shape than the scores, unless ``multi_class``) top1_acc, top5_acc;
        all device tensors (no host sync)."""
        label, with_acc = self._prepare_label(label, cls_score.shape[0])
        out = dict()
        if with_acc:
            with torch.no_grad():
                top = cls_score.topk(min(5, cls_score.shape[1]), dim=1).indices
                hit = top == label.view(-1, 1)
                out = dict(top1_acc=hit[:, 0].double().mean(), top5_acc=hit.any(1).double().mean())
        out['loss_cls'] = self.loss_cls(cls_score, label)
        return out


@HEADS.register_module()
class GCNHead(SimpleHead):

    def __init__(self, num_classes, in_channels, loss_cls=dict(type='CrossEntropyLoss'), dropout=0., init_std=0.01,
                 **kwargs):
        super().__init__(num_classes, in_channels, loss_cls=loss_cls, dropout=dropout, init_std=init_std, mode='GCN',
                         **kwargs)
